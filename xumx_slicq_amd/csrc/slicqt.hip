// Forward / inverse sliced Constant-Q transform for gfx950.
//
// Forward  (closed form, SURVEY.md 8(a) F*; reference nsgt/slicing.py, nsgt/nsgtf.py, nsgt/slicq.py:13-33)
//   seg[bc,s,p]   = tw[p] * xpad[bc, (2s-2)h + p]                         k_slice_window   (HBM stream)
//   U[bc,s,:]     = rfft_L(seg[bc,s,:])                                   rocFFT
//   coef[bc,j,s,:] = U[bc,s, bin0_j : bin0_j+Lg_j] (Hermitian-reflected at DC/Nyquist) x Wf_j
//                                                                         grouped fp32-MFMA GEMM
//   Wf_j = diag(g_j * (-1)^(c_j/2) / Lg_j) * IDFT_Lg, real-ified on interleaved (re,im).
// Inverse  (closed form I2; reference nsgt/nsigtf.py, nsgt/unslicing.py)
//   Z[bc,j,s,:]   = coef[bc,j,s,:] x Wi_j,  Wi_j = DFT_Lg * diag(gd_j * Lg_j * (-1)^(c_j/2) / L)
//   fr[bc,s,k]    = sum over bands covering bin k of Z[bc,j,s,k-bin0_j]   k_spectrum_gather (HBM stream)
//   fr[bc,s,q-c_j] += the mirrored synthesis of a band across DC           k_twin_synthesis (dc_twins.h; plans of xsq_plan_create_twins only)
//   seg[bc,s,:]   = L * irfft_L(fr[bc,s,:])  (unnormalised c2r; the 1/L sits in Wi)   rocFFT
//   y[bc,i]       = seg[bc,s0,i-(2s0-2)h] + seg[bc,s0+1,i-2h*s0],  s0 = i/(2h)        k_overlap_add
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/xumx_slicq_hip.h"
#include "gemm_tile.h"
#include "plan.h"
#include "prof.h"
#include "slice_fft.h"
#include "band_dft4.h"
#include "band_dft4s.h"
#include "dc_twins.h"
#include "band_fft.h"

namespace xsq {

static thread_local char g_err[1024] = "";
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// ------------------------------------------------------------------------------------------
// streaming kernels
// ------------------------------------------------------------------------------------------
// grid (ceil(L/256), BC*S).  Reads x once (each sample lands in two slices), writes seg once.
// ring > 0 (the streaming session, xsq_slicqt_forward_ring): x is a ring of `ring` samples per channel holding absolute sample
// i at i % ring, row (bc, s) is the slice of absolute index s0 + s, and n counts the samples of the whole stream so far; those
// from new0 on are read from xnew and stored to the ring by the slice whose second half holds them (k_slice_rfft, RING).
__global__ __launch_bounds__(256) void k_slice_window(const float* __restrict__ x,
                                                       const float* __restrict__ tw,
                                                       float* __restrict__ seg, int S, int64_t n, int L,
                                                       int h, const int64_t* __restrict__ xrows = nullptr,
                                                       const float* const* __restrict__ xslot = nullptr,
                                                       int64_t s0 = 0, int ring = 0, float* ring_w = nullptr,
                                                       const float* __restrict__ xnew = nullptr, int64_t new0 = 0,
                                                       int64_t new_stride = 0) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= L) return;
    const int row = blockIdx.y;  // bc*S + s
    const int bc = row / S, s = row - bc * S;
    const int64_t i = (2 * (s0 + s) - 2) * h + p;
    float v = 0.f;
    if (ring) {
        if (i >= 0 && i < n) {
            const int64_t r = (int64_t)bc * ring + i % ring;
            const float xv = i >= new0 ? xnew[(int64_t)bc * new_stride + i - new0] : x[r];
            if (i >= new0 && p >= 2 * h) ring_w[r] = xv;
            v = tw[p] * xv;
        }
    } else if (i >= 0 && i < n) v = tw[p] * (xslot ? *xslot : x)[(xrows ? xrows[bc] : (int64_t)bc * n) + i];
    seg[(int64_t)row * L + p] = v;
}

// grid (ceil(nbins/256), BC*S).  fr[row][k] = sum of the covering bands' synthesis outputs.
__global__ __launch_bounds__(256) void k_spectrum_gather(const float* __restrict__ Z,
                                                          const BandDev* __restrict__ bands,
                                                          const int* __restrict__ cov_ptr,
                                                          const int* __restrict__ cov_band,
                                                          float2* __restrict__ fr, int BC, int S, int nbins) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= nbins) return;
    const int row = blockIdx.y;
    const int bc = row / S, s = row - bc * S;
    const int64_t BCS = (int64_t)BC * S;
    float2 acc = make_float2(0.f, 0.f);
    for (int e = cov_ptr[k]; e < cov_ptr[k + 1]; ++e) {
        const BandDev b = bands[cov_band[e]];
        const int64_t off = 2 * (BCS * b.cum + (((int64_t)bc * b.F + b.f) * S + s) * b.Lg + (k - b.bin0));
        const float2 z = *reinterpret_cast<const float2*>(Z + off);
        acc.x += z.x;
        acc.y += z.y;
    }
    // irfft ignores the imaginary part of the DC and Nyquist bins (torch.fft.irfft, nsigtf.py:103)
    if (k == 0 || k == nbins - 1) acc.y = 0.f;
    fr[(int64_t)row * nbins + k] = acc;
}

// grid (ceil(length/256), BC).  Each output sample is the sum of exactly two slices.
__global__ __launch_bounds__(256) void k_overlap_add(const float* __restrict__ seg, float* __restrict__ y,
                                                      const int64_t* __restrict__ row_off,
                                                      int S, int64_t length, int L, int h) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= length) return;
    const int bc = blockIdx.y;
    const int s0 = (int)(i / (2 * h));
    const int p1 = (int)(i - (int64_t)2 * h * s0);  // position inside slice s0+1
    const float* base = seg + (int64_t)bc * S * L;
    float v = base[(int64_t)s0 * L + p1 + 2 * h];
    if (s0 + 1 < S) v += base[(int64_t)(s0 + 1) * L + p1];
    y[(row_off ? row_off[bc] : (int64_t)bc * length) + i] = v;
}

// k_overlap_add with every slice multiplied by the slice window first (the adjoint of the forward transform on the rocFFT
// path; the hand-written slice FFT does the same in its WINDOW instantiation).  Same grid, same order of the two terms.
__global__ __launch_bounds__(256) void k_overlap_add_windowed(const float* __restrict__ seg, const float* __restrict__ tw,
                                                               float* __restrict__ y, int S, int64_t length, int L, int h) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= length) return;
    const int bc = blockIdx.y;
    const int s0 = (int)(i / (2 * h));
    const int p1 = (int)(i - (int64_t)2 * h * s0);
    const float* base = seg + (int64_t)bc * S * L;
    float v = tw[p1 + 2 * h] * base[(int64_t)s0 * L + p1 + 2 * h];
    if (s0 + 1 < S) v += tw[p1] * base[(int64_t)(s0 + 1) * L + p1];
    y[(int64_t)bc * length + i] = v;
}

// The fold of the adjoint of the forward transform (xsq_slicqt_forward_adjoint).  The analysis reads the bins outside
// [0, L/2] of a band next to DC or Nyquist from the Hermitian mirror, conjugated; its adjoint therefore adds the conjugate
// of what the synthesis kernels left on such an entry of Z (the inverse transform drops it) to the mirrored bin.  Here it is
// added onto an entry of Z that the gather sums into that bin anyway, so the gather schedule -- and the disjointness of the
// bands of a phase it rests on -- stays as it is.  One lane per destination entry, its sources in table order: no atomics,
// the same bits every run.  No source is a destination.  grid (rows), Z in the arena's layout (the rocFFT path's; the
// hand-written slice FFT folds inside its own kernel, slice_fft.h: FOLD -- measured 3 to 5 % of the call faster than this pass in
// front of it, profiles/autograd_fold_ab.jsonl).
struct FoldDst { int jd, pd, first, count; };     // band and spectrum position (bin = bin0 + p) of the destination; its sources
struct FoldSrc { int js, ps; };
__global__ __launch_bounds__(256) void k_fold_mirrored(float* __restrict__ Z, const BandDev* __restrict__ bands,
                                                        const FoldDst* __restrict__ dst, const FoldSrc* __restrict__ src, int ndst,
                                                        int BC, int S) {
    const int row = blockIdx.x;
    const int bc = row / S, s = row - bc * S;
    const int64_t BCS = (int64_t)BC * S;
    auto at = [&](int j, int p) {
        const BandDev b = bands[j];
        const int64_t e = BCS * b.cum + (((int64_t)bc * b.F + b.f) * S + s) * b.Lg + p;
        return reinterpret_cast<float2*>(Z) + e;
    };
    for (int i = threadIdx.x; i < ndst; i += 256) {
        const FoldDst d = dst[i];
        float2* const zd = at(d.jd, d.pd);
        float2 acc = *zd;
        for (int e = d.first; e < d.first + d.count; ++e) {
            const float2 z = *at(src[e].js, src[e].ps);
            acc.x += z.x;
            acc.y -= z.y;
        }
        *zd = acc;
    }
}

// The overlap-add of a streaming step over the S new slices of the step (CarryArgs, slice_fft.h): grid (ceil((nblk + 1) * 2h
// / 256), BC).  Block b of the step = second half of position b (slice b - shift, or the carried half when there is none) +
// first half of position b + 1, summed in the order of k_overlap_add; block nblk is the new carry.
__global__ __launch_bounds__(256) void k_overlap_add_carry(const float* __restrict__ seg, float* __restrict__ y, const CarryArgs C,
                                                            int S, int64_t length, int L, int h) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int h2 = 2 * h;
    if (i >= (C.nblk + 1) * h2) return;
    const int bc = blockIdx.y;
    const int blk = i / h2, p1 = i - blk * h2;
    const float* base = seg + (int64_t)bc * S * L;
    const int sa = blk - C.shift, sb = sa + 1;      // the slices whose second / first half meet in this block
    float v = sa >= 0 ? base[(int64_t)sa * L + p1 + h2] : C.carry_in[(int64_t)bc * h2 + p1];
    if (blk >= C.nblk) { C.carry_out[(int64_t)bc * h2 + p1] = v; return; }
    if (sb < S) v += base[(int64_t)sb * L + p1];
    if (i < length) y[(int64_t)bc * C.out_stride + i] = v;
}

// Slices [s0, s0 + Sdst) of an arena of Ssrc slices as an arena of Sdst slices (the new slices of a streaming step out of the
// window the CDAE ran on): block j holds [C][F][S][T] entries of cplx floats from C * S * cum_j on.  grid (ceil(per / 1024), nblocks, C).
constexpr int TAKE_MAX_BLOCKS = 256;
struct TakeArgs {
    const float* src[2];                // the complex mix arena (C[0] channels), the real mask arena (C[1] channels): one launch
    float* dst[2];
    int C[2];
    int Ssrc, Sdst, s0;
    int cum[TAKE_MAX_BLOCKS + 1];       // coefficients per channel-slice before block j
    int T[TAKE_MAX_BLOCKS];
};

// grid (ceil(2 * per / 1024), nblocks, C[0] + C[1])
__global__ __launch_bounds__(256) void k_take_slices(TakeArgs a) {
    const int j = blockIdx.y;
    const int which = (int)blockIdx.z < a.C[0] ? 0 : 1, ch = blockIdx.z - (which ? a.C[0] : 0), C = a.C[which], cplx = which ? 1 : 2;
    const int Tc = a.T[j] * cplx;                                    // floats of one (f, s) row (% 4 == 0: T % 4 == 0)
    const int FT = (a.cum[j + 1] - a.cum[j]) * cplx;                 // F * Tc
    const int64_t e = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (e >= (int64_t)a.Sdst * FT) return;
    const int row = (int)(e / Tc), t = (int)(e - (int64_t)row * Tc); // row = f * Sdst + s
    const int f = row / a.Sdst, s = row - f * a.Sdst;
    const float* src = a.src[which] + ((int64_t)C * a.cum[j] * cplx + (int64_t)ch * FT) * a.Ssrc + ((int64_t)f * a.Ssrc + a.s0 + s) * Tc + t;
    float* dst = a.dst[which] + ((int64_t)C * a.cum[j] * cplx + (int64_t)ch * FT) * a.Sdst + e;
    *reinterpret_cast<float4*>(dst) = *reinterpret_cast<const float4*>(src);
}

// ------------------------------------------------------------------------------------------
// grouped GEMM operators
// ------------------------------------------------------------------------------------------
struct BandGroup {
    int M, N, K, ldb;
    const float* B;
    int Lg, bin0, f, F;
    int64_t base;  // float offset of (bc=0, f, s=0) of this band in the arena
    int64_t cum;   // complex coefficients per channel-slice before this band's block
    int j;         // band index inside the plan
};

// coef = U_window x Wf
struct BandFwdOp {
    typedef BandGroup Group;
    struct RowA {
        const float* p;  // U row (bc,s), nullptr when past M
    };
    const float* U;
    float* coef;
    const BandDev* bands;
    const float* W;
    int BC, S, nbins, L;
    float* xin;            // optional whitened magnitude beside the coefficients (see Band4Args)
    const float* mean;
    const float* scale;
    int split;

    __device__ Group group(int j) const {
        const BandDev b = bands[j];
        Group g;
        g.M = BC * S; g.N = 2 * b.Lg; g.K = 2 * b.Lg; g.ldb = b.ldw; g.B = W + b.w_off;
        g.Lg = b.Lg; g.bin0 = b.bin0; g.f = b.f; g.F = b.F;
        g.base = 2 * ((int64_t)BC * S * b.cum + (int64_t)b.f * S * b.Lg);
        g.cum = b.cum;
        g.j = j;
        return g;
    }
    __device__ RowA row_a(const Group& g, int m) const {
        RowA r;
        r.p = m < g.M ? U + (int64_t)m * 2 * nbins : nullptr;
        return r;
    }
    // two complex bins per call; bins outside [0, L/2] come from the Hermitian mirror (their
    // conjugation is folded into the signs of Wf's imaginary rows)
    __device__ float4 load_a4(const Group& g, const RowA& r, int k) const {
        const bool ok = r.p != nullptr && k < g.K;                       // out of range: both loads read zero16()
        int i0 = g.bin0 + (k >> 1), i1 = i0 + 1;
        i0 = i0 < 0 ? -i0 : (i0 > L / 2 ? L - i0 : i0);
        i1 = i1 < 0 ? -i1 : (i1 > L / 2 ? L - i1 : i1);
        const float2 a = *reinterpret_cast<const float2*>(ok ? r.p + 2 * i0 : zero16());
        const float2 b = *reinterpret_cast<const float2*>(ok ? r.p + 2 * i1 : zero16());
        return make_float4(a.x, a.y, b.x, b.y);
    }
    __device__ void epilogue(const Group& g, int row0, int n, const f32x16& a0, const f32x16& a1, bool wide) const {
        const bool c0 = n < g.N, c1 = wide && n + 32 < g.N;
        int bc = row0 / S, s = row0 - bc * S;          // one division per lane, then carry
        int prev = 0;
        // loaded BEFORE the first store: a load between two stores makes the compiler wait for the store as well
        const float mu = xin ? mean[g.j] : 0.f, sc = xin ? scale[g.j] : 1.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            s += acc_row(r) - prev; prev = acc_row(r);
            while (s >= S) { s -= S; ++bc; }
            if (row0 + acc_row(r) >= g.M) break;
            float* d = coef + g.base + ((int64_t)bc * g.F * S + s) * (2 * g.Lg) + n;
            if (c0) d[0] = a0[r];
            if (c1) d[32] = a1[r];
            if (xin) {       // uniform.  Column n = 2t + (re/im): the even lane of a pair forms |c| and stores it
                const float o0 = __shfl_xor(a0[r], 1), o1 = __shfl_xor(a1[r], 1);
                if (!(n & 1)) {
                    float* x = xin + ((d - coef) >> 1);
                    if (c0) { float v = whiten_mag(a0[r], o0, mu, sc); if (split) v = bf3_word(v); x[0] = v; }
                    if (c1) { float v = whiten_mag(a1[r], o1, mu, sc); if (split) v = bf3_word(v); x[16] = v; }
                }
            }
        }
    }
};

// The analysis of the bands above the radix-4 kernels' Lg = 320 (4 * D4_MPAD; none in Bark-262 or Mel-32): BandFwdOp's
// product with the sum over K = 2 Lg carried in float64 on the vector ALU.  On the tile engine one fp32 MFMA accumulator
// chain takes all K products of an output; a DC band is a plateau of ones, and where the phases of the slice spectrum
// align its terms add with one sign: measured on `bark, 400, 300` (Lg 376, K = 752) that chain is off by 7e-6 of the
// coefficient, 22 times the fp32 FFT of the same band.  A product of two floats is exact in float64 and 752 of them sum
// there to 1e-13, so the result is the float64 sum rounded once.  Tile = 32 rows x 64 columns, K-step 16, thread (ty, tx)
// = rows ty and ty + 16, columns 4 tx .. 4 tx + 3 (two complex coefficients, so the whitened magnitude needs no
// exchange); operands, loaders, arena layout and the xin epilogue are BandFwdOp's.  Fixed order: the same bits every run.
constexpr int LONG_LG = 4 * D4_MPAD, LONG_BM = 32;
__global__ __launch_bounds__(256) void k_band_fwd_long(const BandFwdOp op, const TileDev* __restrict__ tiles) {
    __shared__ __attribute__((aligned(16))) float As[LONG_BM][20];
    __shared__ __attribute__((aligned(16))) float Bs[16][68];
    const TileDev t = tiles[blockIdx.x];
    const BandGroup g = op.group(t.group);
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int s_row = tid >> 2, s_kq = (tid & 3) * 4;
    const BandFwdOp::RowA ra = op.row_a(g, s_row < LONG_BM ? t.m0 + s_row : g.M);
    const float* bt = g.B + (int64_t)(t.n0 + s_row) * g.ldb + s_kq;      // Wt[n][k], padded to whole tiles with zeros
    double acc[2][4] = {{0., 0., 0., 0.}, {0., 0., 0., 0.}};
    for (int k0 = 0; k0 < g.K; k0 += 16) {
        const float4 b = *reinterpret_cast<const float4*>(bt + k0);
        if (s_row < LONG_BM) *reinterpret_cast<float4*>(&As[s_row][s_kq]) = op.load_a4(g, ra, k0 + s_kq);
        Bs[s_kq][s_row] = b.x; Bs[s_kq + 1][s_row] = b.y; Bs[s_kq + 2][s_row] = b.z; Bs[s_kq + 3][s_row] = b.w;
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
            const float4 w = *reinterpret_cast<const float4*>(&Bs[kk][4 * tx]);
            const double wd[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const double a = As[ty + 16 * r][kk];
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[r][c] = fma(a, wd[c], acc[r][c]);
            }
        }
        __syncthreads();
    }
    const int n = t.n0 + 4 * tx;
    if (n >= g.N) return;                                                // N = 2 Lg is a multiple of 8
    const float mu = op.xin ? op.mean[g.j] : 0.f, sc = op.xin ? op.scale[g.j] : 1.f;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int m = t.m0 + ty + 16 * r;
        if (m >= g.M) continue;
        const int bc = m / op.S, s = m - bc * op.S;
        const float4 v = make_float4((float)acc[r][0], (float)acc[r][1], (float)acc[r][2], (float)acc[r][3]);
        float* d = op.coef + g.base + ((int64_t)bc * g.F * op.S + s) * (2 * g.Lg) + n;
        *reinterpret_cast<float4*>(d) = v;                               // 16-byte aligned: Lg % 4 == 0, n % 4 == 0
        if (op.xin) {
            float x0 = whiten_mag(v.x, v.y, mu, sc), x1 = whiten_mag(v.z, v.w, mu, sc);
            if (op.split) { x0 = bf3_word(x0); x1 = bf3_word(x1); }
            *reinterpret_cast<float2*>(op.xin + ((d - op.coef) >> 1)) = make_float2(x0, x1);
        }
    }
}

// Z = coef x Wi   (dense rows in, dense rows out, same arena layout)
struct BandInvOp {
    typedef BandGroup Group;
    struct RowA {
        const float* p;
        const float* mk;
    };
    const float* coef;
    float* Z;
    const BandDev* bands;
    const float* W;
    int BC, S;
    int row_len;   // > 0: write row-major, phase-ordered (rows of row_len complex entries) for k_slice_irfft
    const float* mask;   // optional: coefficients = mask * mix (see Band4Args); coef is then the mix arena, BCx channels
    int BCx;

    __device__ Group group(int j) const {
        const BandDev b = bands[j];
        Group g;
        g.M = BC * S; g.N = 2 * b.Lg; g.K = 2 * b.Lg; g.ldb = b.ldw; g.B = W + b.w_off;
        g.Lg = b.Lg; g.bin0 = b.ent; g.f = b.f; g.F = b.F;   // bin0 slot carries the entry offset here
        g.base = 2 * ((int64_t)BC * S * b.cum + (int64_t)b.f * S * b.Lg);
        g.cum = b.cum;
        return g;
    }
    __device__ int64_t row_off(const Group& g, int m) const {
        const int bc = m / S, s = m - bc * S;
        return g.base + ((int64_t)bc * g.F * S + s) * (2 * g.Lg);
    }
    __device__ RowA row_a(const Group& g, int m) const {
        RowA r;
        r.p = nullptr; r.mk = nullptr;
        if (m >= g.M) return r;
        if (!mask) { r.p = coef + row_off(g, m); return r; }
        const int bc = m / S, s = m - bc * S;
        r.mk = mask + row_off(g, m) / 2;
        r.p = coef + 2 * ((int64_t)BCx * S * g.cum + (int64_t)g.f * S * g.Lg) + ((int64_t)(bc % BCx) * g.F * S + s) * (2 * g.Lg);
        return r;
    }
    __device__ float4 load_a4(const Group& g, const RowA& r, int k) const {
        const bool ok = r.p != nullptr && k < g.K;
        return *reinterpret_cast<const float4*>(ok ? r.p + k : zero16());  // rows are 32-byte aligned (Lg % 4 == 0)
    }
    // masked synthesis: the two masks of the K-chunk travel beside the coefficients and are applied when the
    // K-step goes into LDS (gemm_tile.h, aux hook)
    typedef float2 Aux;
    __device__ Aux load_aux(const Group& g, const RowA& r, int k) const {
        const bool ok = r.mk != nullptr && k < g.K;
        return *reinterpret_cast<const float2*>(ok ? r.mk + (k >> 1) : zero16());
    }
    __device__ float4 finish(float4 v, const Aux& mk) const {
        if (mask) { v.x *= mk.x; v.y *= mk.x; v.z *= mk.y; v.w *= mk.y; }      // uniform
        return v;
    }
    __device__ void epilogue(const Group& g, int row0, int n, const f32x16& a0, const f32x16& a1, bool wide) const {
        const bool c0 = n < g.N, c1 = wide && n + 32 < g.N;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = row0 + acc_row(r);
            if (m >= g.M) break;
            float* d = (row_len ? Z + 2 * ((int64_t)m * row_len + g.bin0) : Z + row_off(g, m)) + n;
            if (c0) d[0] = a0[r];
            if (c1) d[32] = a1[r];
        }
    }
};

// Gain-weighted sums of the four targets (xsq_slicqt_inverse_remix): dst channel (r, ch) = sum_t g[r][t] * src channel
// (t, ch), element by element, t = 0..3 in this fixed order.  Arena layout (any channel count C): band block j holds
// [C][S * F_j * T_j] coefficients from C * S * cum_j on -- so the element e of channel ch in block j sits at the same e
// in both arenas, only the block bases and channel strides differ.  src has 4 * nch channels, dst R * nch.  Masks are
// real (cplx = 1), estimates complex (cplx = 2).  A target no row weights (use[t] == 0) is not loaded: a uniform branch
// on a kernel argument.  Products are rounded before the sum (contraction off): a one-hot row copies its target's bits.
constexpr int REMIX_MAX_BLOCKS = 256;      // (Bark-262: 70 blocks; the arguments stay near 1.1 KB)
struct RemixArgs {
    const float* src;
    float* dst;
    int nch, R, S, cplx;
    float g[4][4];
    int use[4];
    int cum[REMIX_MAX_BLOCKS + 1];      // coefficients per channel-slice before block j (cum[nblocks] = sumFT)
};

__global__ __launch_bounds__(256) void k_remix_combine(RemixArgs a) {
#pragma clang fp contract(off)
    const int j = blockIdx.y, ch = blockIdx.z;
    const int64_t per = (int64_t)a.S * (a.cum[j + 1] - a.cum[j]) * a.cplx;     // floats of one channel in block j (% 4 == 0: T % 4 == 0)
    const int64_t e = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (e >= per) return;
    const int64_t base = (int64_t)a.S * a.cum[j] * a.cplx;                    // floats of one channel before block j
    const float* s = a.src + base * (4 * a.nch) + (int64_t)ch * per + e;
    float4 m[4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
        m[t] = a.use[t] ? *reinterpret_cast<const float4*>(s + (int64_t)t * a.nch * per) : make_float4(0.f, 0.f, 0.f, 0.f);
    float* d = a.dst + base * ((int64_t)a.R * a.nch) + (int64_t)ch * per + e;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (r >= a.R) break;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (!a.use[t]) continue;
            const float g = a.g[r][t];
            acc.x = acc.x + g * m[t].x; acc.y = acc.y + g * m[t].y; acc.z = acc.z + g * m[t].z; acc.w = acc.w + g * m[t].w;
        }
        *reinterpret_cast<float4*>(d + (int64_t)r * a.nch * per) = acc;
    }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
// dense-GEMM tiles: all bands, or only the short ones when the radix-4 kernel takes the rest
// part (the table's `sub`): 0 every such band (the synthesis; the analysis of a plan with no band above LONG_LG, so such a
// plan keeps its one table), 1 the analysis' bands up to LONG_LG, 2 the tiles of k_band_fwd_long over the bands above it
static int get_band_tiles(xsq_plan* P, int rows, TileTable* out, int part = 0) {
    const bool r4 = P->band_radix4 && P->nbands4 > 0;
    const auto is_long = [&](int j) { return P->bands[j].Lg > LONG_LG && !P->on_fft[j]; };
    bool any_long = false;
    for (int j = 0; j < P->nbands; ++j) any_long = any_long || is_long(j);
    if (!any_long) {
        if (part == 2) { *out = TileTable{}; return XSQ_OK; }
        part = 0;
    }
    return cached_tiles<TileDev>(P->mu, P->tiles, TileKey{TileKind::BandGemm, rows, 0, part, r4 ? 1 : 0}, out, [&](std::vector<TileDev>& t) {
        // longest tiles first (K = 2*Lg grows along the band table): the launch ends on short tiles
        const auto push = [&](int j) {
            if (P->on_fft[j]) return;               // (band_fft.h: no dense matrix)
            if (part == 2) { if (is_long(j)) push_group_tiles(t, j, rows, 2 * P->bands[j].Lg, LONG_BM); }
            else if (part == 0 || !is_long(j)) push_group_tiles(t, j, rows, 2 * P->bands[j].Lg);
        };
        if (r4) {
            for (int i = (int)P->bands4_small.size() - 1; i >= 0; --i) push(P->bands4_small[i]);
        } else {
            for (int j = P->nbands - 1; j >= 0; --j) push(j);
        }
    });
}

// Bands at least this long take the radix-4 kernel, shorter ones the dense engine.  Measured with the full-width kernel
// (r03o, sum of the four band kernels): 64 -> 1.53 ms, 48 -> 1.485, 32 -> 1.49, 16 -> 1.53; again with the buffer-addressed
// kernel (r4f, four full chunks): 48 -> 1.285 ms, 40 -> 1.272, 32 -> 1.280, 24 -> 1.252, 16 -> 1.304.
#ifndef XSQ_D4_MIN_LG_DEFAULT
#define XSQ_D4_MIN_LG_DEFAULT 24
#endif

// Process switches, read once (a function-local static: initialised under the language's lock).
//   XSQ_D4_SYM=0      the complex-product radix-4 kernel (band_dft4.h) instead of the pair-contracted default (band_dft4s.h);
//                     tests/test_slicqt_gpu.py holds the two arms together
//   XSQ_D4_MIN_LG=n   bands at least n (>= 16) long take the radix-4 kernel, shorter ones the dense engine: the split point
//                     behind XSQ_D4_MIN_LG_DEFAULT, which bench.py reads for its flop split
struct Switches {
    bool d4_sym = true;
    int d4_min_lg = XSQ_D4_MIN_LG_DEFAULT;
    Switches() {
        if (const char* e = getenv("XSQ_D4_SYM")) d4_sym = atoi(e) != 0;
        if (const char* e = getenv("XSQ_D4_MIN_LG")) d4_min_lg = atoi(e) >= 16 ? atoi(e) : d4_min_lg;
    }
};
static const Switches& switches() { static const Switches sw; return sw; }

// tiles of the radix-4 kernels: 32 rows x every column of the band; TileDev.narrow = number of 16-column blocks -- of the
// band's 2m columns (band_dft4.h), or with `sym` of its outputs k = 0 .. m / 2 (band_dft4s.h).
// `share` > 0 (masked synthesis): rows r and r + share, r + 2*share, ... read the same mix rows (the targets of one
// (sample, channel, slice)); their tiles are made neighbours so the mix is fetched once per XCD.  When share is not a
// multiple of the tile height the last tile of a copy runs into the next copy's first rows and recomputes them
// (same values, written twice).
static int get_dft4_full_tiles(xsq_plan* P, int rows, TileTable* out, int share, bool sym) {
    return cached_tiles<Tile4Dev>(P->mu, P->tiles, TileKey{TileKind::Dft4Full, rows, share, 0, sym ? 1 : 0}, out, [&](std::vector<Tile4Dev>& t) {
        const Band4Dev* b4 = reinterpret_cast<const Band4Dev*>(P->bands4_host.data());
        const int span = share > 0 ? share : rows, copies = share > 0 ? rows / share : 1;
        for (int i = P->nbands4 - 1; i >= 0; --i) {
            int ncb = (2 * P->bands4_m[i] + 15) / 16;
            if (sym) ncb = (P->bands4_m[i] / 2 + 1 + 15) / 16;        // band_dft4s.h: blocks of the outputs k = 0 .. m / 2
            for (int m0 = 0; m0 < span; m0 += D4H_ROWS)
                for (int k = 0; k < copies; ++k) t.push_back(Tile4Dev{m0 + k * span, ncb, b4[i]});
        }
    });
}

// The radix-4 band kernel reaches operands and results through buffer descriptors per band block / tile with 32-bit byte
// offsets and switches lanes off with offsets of 2^30 and 2^31 (band_dft4.h, common.h): every such range stays below 2^30
// bytes.  Checked where a transform call enters, before anything is launched.
static int d4_ranges_ok(const xsq_plan* P, int64_t rows, const char* who) {
    if (!(P->band_radix4 && P->nbands4)) return XSQ_OK;
    XSQ_REQUIRE(8 * rows * P->d4_max_block < (1ll << 30) && (int64_t)8 * D4H_ROWS * std::max<int64_t>(P->nbins, P->sumFT) < (1ll << 30),
                "%s: %lld rows x %lld coefficients of a band block exceed 2^30 bytes; split the call (fewer stacked chunks)",
                who, (long long)rows, (long long)P->d4_max_block);
    return XSQ_OK;
}

// The radix-4 band kernel over every eligible band, in one launch: the pair-contracted form (band_dft4s.h), or with
// XSQ_D4_SYM=0 the complex-product form (band_dft4.h) in its 10-block instantiation (three workgroups per CU).  A masked
// synthesis takes the instantiation that multiplies the mask in.
template <bool FWD>
static int launch_dft4(xsq_plan* P, const Band4Args& a4, int rows, int share, hipStream_t stream) {
    const bool sym = switches().d4_sym;
    const bool masked = !FWD && a4.mask != nullptr;
    TileTable t;
    if (int rc = get_dft4_full_tiles(P, rows, &t, share, sym)) return rc;
    if (!t.ntiles) return XSQ_OK;
    auto kernel = masked ? band_dft4s_kernel<false, true> : band_dft4s_kernel<FWD, false>;
    if (!sym) kernel = masked ? band_dft4_full_kernel<false, 10, true> : band_dft4_full_kernel<FWD, 10, false>;
    hipLaunchKernelGGL(kernel, dim3(t.ntiles), dim3(sym ? 256 : D4H_NT), 0, stream, a4, (const Tile4Dev*)t.d_tiles, t.ntiles);
    return XSQ_OK;
}

static int get_fft(xsq_plan* P, int inverse, int batch, FftPlan* out) {
    std::lock_guard<std::mutex> lk(P->mu);
    auto key = std::make_pair(inverse, batch);
    auto it = P->fft.find(key);
    if (it != P->fft.end()) {
        *out = it->second;
        return XSQ_OK;
    }
    static std::once_flag once;
    std::call_once(once, [] { rocfft_setup(); });
    FftPlan f;
    size_t len = (size_t)P->L;
    rocfft_status st = rocfft_plan_create(&f.plan, rocfft_placement_notinplace,
                                          inverse ? rocfft_transform_type_real_inverse
                                                  : rocfft_transform_type_real_forward,
                                          rocfft_precision_single, 1, &len, (size_t)batch, nullptr);
    if (st != rocfft_status_success) {
        set_error("rocfft_plan_create(L=%d, batch=%d, inverse=%d) failed: %d", P->L, batch, inverse, (int)st);
        return XSQ_ERR_FFT;
    }
    rocfft_plan_get_work_buffer_size(f.plan, &f.work_bytes);
    if (rocfft_execution_info_create(&f.info) != rocfft_status_success) {
        set_error("rocfft_execution_info_create failed");
        return XSQ_ERR_FFT;
    }
    P->fft[key] = f;
    *out = f;
    return XSQ_OK;
}

static int run_fft(const FftPlan& f, void* in, void* out, void* work, hipStream_t stream) {
    if (rocfft_execution_info_set_stream(f.info, stream) != rocfft_status_success) {
        set_error("rocfft_execution_info_set_stream failed");
        return XSQ_ERR_FFT;
    }
    if (f.work_bytes) {
        if (rocfft_execution_info_set_work_buffer(f.info, work, f.work_bytes) != rocfft_status_success) {
            set_error("rocfft_execution_info_set_work_buffer failed");
            return XSQ_ERR_FFT;
        }
    }
    void* ib[1] = {in};
    void* ob[1] = {out};
    rocfft_status st = rocfft_execute(f.plan, ib, ob, f.info);
    if (st != rocfft_status_success) {
        set_error("rocfft_execute failed: %d", (int)st);
        return XSQ_ERR_FFT;
    }
    return XSQ_OK;
}

// (a plan with the mirrored synthesis adds it to the slice spectra in memory, dc_twins.h: rocFFT whatever L is; so does a plan
// with a band on the FFT band engine, which writes Z in the arena's layout, band_fft.h)
static inline bool lds_fft(const xsq_plan* P) {
    return P->fft_backend == 0 && P->L == FFT_L && P->d_tgt != nullptr && P->ntwins == 0 && P->nlong == 0;
}
static inline FftTables fft_tables(const xsq_plan* P) {
    return FftTables{P->d_T, P->d_T + FFT_R1 * FFT_M1, P->d_T + FFT_R1 * FFT_M1 + FFT_R2 * FFT_R3};
}

// ------------------------------------------------------------------------------------------
// plan creation: one function per family of tables; plan_build calls them in order and uploads what they made
// ------------------------------------------------------------------------------------------
constexpr double PI2 = 6.283185307179586476925286766559;

// The short bands inside k_slice_irfft (slice_fft.h, SHORT): their transformed windows wait in LDS from this spectrum bin on,
// above every short band and below the end of the slice spectrum, and one launch holds at most this many radix-4
// butterflies, small DFTs and scratch entries per gather phase (the kernel's U1 / U2 / UG register arrays).
constexpr int SHORT_SCRATCH0 = 4096;
constexpr int SHORT_MAX_BUTTERFLIES = 1280, SHORT_MAX_DFTS = 768, SHORT_MAX_PHASE_ENTRIES = 1280;
// The four-phases-in-flight gather of k_slice_irfft (slice_fft.h, FAST4) holds one phase as entry pairs in registers: this
// many entries at 512 threads (the kernel's UP pairs per lane).
constexpr int FAST4_MAX_PHASE_ENTRIES = 2 * 512 * ((4864 / 2 + 1 + 511) / 512);

// The arguments of xsq_plan_create, and what more than one stage derives from them.
struct PlanArgs {
    int L, tr, nbands;
    const int32_t *Lg, *c;
    const float* g;
    const double* gd;
    const float* tw;
    std::vector<int64_t> g_off;     // first sample of band j's windows inside g / gd (the bands' windows lie back to back)
    const double* ga64 = nullptr;   // when set: the analysis window in double, in place of g (the adjoint tables, adjoint_tables())
    const double* gs64 = nullptr;   // when set: the synthesis window without its sign, in place of gd Lg / L (forward_adjoint_tables())

    // (-1)^(c_j / 2), and sample q of the band's two windows with the sign and the transform's scale folded in.  The dense
    // matrices, the window pool of the radix-4 kernel and the short-band schedule all take them from here: the engines are
    // interchangeable per band only while these agree to the bit.
    double sign(int j) const { return ((c[j] / 2) % 2 == 0) ? 1.0 : -1.0; }
    double analysis_window(int j, int q) const { return (ga64 ? ga64[g_off[j] + q] : (double)g[g_off[j] + q]) * sign(j) / Lg[j]; }
    double synthesis_window(int j, int q) const { return gs64 ? gs64[g_off[j] + q] * sign(j) : gd[g_off[j] + q] * Lg[j] * sign(j) / L; }
};

// blocks = runs of equal band length (nsgt/nsgtf.py:66-78), and the band table (without .ent: build_slice_fft_tables)
static int build_band_tables(xsq_plan* P, const PlanArgs& A) {
    const int L = A.L, nbands = A.nbands;
    const int32_t *Lg = A.Lg, *c = A.c;
    P->L = L; P->tr = A.tr; P->h = L / 4; P->nbins = L / 2 + 1; P->nbands = nbands;
    int64_t cum = 0;
    for (int j = 0; j < nbands;) {
        int k = j;
        while (k + 1 < nbands && Lg[k + 1] == Lg[j]) ++k;
        P->blocks.push_back(BlockHost{j, k - j + 1, Lg[j], cum});
        cum += (int64_t)(k - j + 1) * Lg[j];
        j = k + 1;
    }
    P->nblocks = (int)P->blocks.size();
    P->sumFT = cum;
    int64_t woff = 0;
    P->on_fft.assign(nbands, 0);
    for (const BlockHost& b : P->blocks) {
        for (int f = 0; f < b.F; ++f) {
            const int j = b.first_band + f;
            if (Lg[j] % 4 != 0 || c[j] % 2 != 0 || Lg[j] > L / 2) {
                set_error("xsq_plan_create: band %d has Lg=%d c=%d (need Lg%%4==0, c even, Lg<=L/2)", j, Lg[j], c[j]);
                return XSQ_ERR_ARG;
            }
            // a long_bands plan: every band above LONG_LG on the FFT band engine (band_fft.h), which has no dense matrix
            P->on_fft[j] = P->long_bands && Lg[j] > LONG_LG;
            XSQ_REQUIRE(!P->on_fft[j] || Lg[j] <= LF_MAX_LG, "xsq_plan_create_flags: band %d has Lg=%d, longer than the FFT band engine's "
                        "maximum %d (XSQ_PLAN_LONG_BANDS, xsq_plan_long_band_max): plan refused", j, Lg[j], LF_MAX_LG);
            BandDev d;
            d.Lg = Lg[j]; d.bin0 = c[j] - Lg[j] / 2; d.f = f; d.F = b.F; d.cum = b.cum;
            d.ldw = (int)round_up(2 * Lg[j], 16); d.w_off = woff; d.ent = 0;
            if (!P->on_fft[j]) woff += round_up(2 * Lg[j], 64) * d.ldw;
            P->bands.push_back(d);
        }
    }
    P->wf_floats = (size_t)woff;
    return XSQ_OK;
}

// Per-band real-ified DFT matrices of the dense engine, stored transposed, Wt[n][k] (K contiguous, as the tile engine wants
// its B operand).
// analysis: k = 2p+ri over the band's window in spectrum order (bin = bin0 + p, window
// index q = (p + Lg/2) mod Lg since windows are stored peak-at-0), n = 2t+ro over coefficients;
// synthesis: k = 2t+ri over coefficients, n = 2p+ro over spectrum positions.
static void build_dense_matrices(const xsq_plan* P, const PlanArgs& A, std::vector<float>& Wf, std::vector<float>& Wi) {
    const size_t floats = P->wf_floats;           // (build_band_tables: the matrices of every band but those of the FFT band engine)
    Wf.assign(floats, 0.f);
    Wi.assign(floats, 0.f);
    for (int j = 0; j < A.nbands; ++j) {
        if (P->on_fft[j]) continue;
        const BandDev& d = P->bands[j];
        const int n = d.Lg, ld = d.ldw;
        std::vector<double> cs(n), sn(n);
        for (int r = 0; r < n; ++r) { cs[r] = std::cos(PI2 * r / n); sn[r] = std::sin(PI2 * r / n); }
        float* wf = Wf.data() + d.w_off;
        float* wi = Wi.data() + d.w_off;
        for (int p = 0; p < n; ++p) {
            const int q = (p + n / 2) % n;
            const int bin = d.bin0 + p;
            const double conj = (bin < 0 || bin > A.L / 2) ? -1.0 : 1.0;  // mirrored bin: input is conj(U)
            const double ga = A.analysis_window(j, q);
            const double gs = A.synthesis_window(j, q);
            for (int t = 0; t < n; ++t) {
                const int r = (int)(((int64_t)q * t) % n);
                // analysis: w = ga * e^{+i 2 pi q t / n};  (a_re + i conj a_im) * w
                const double wr = ga * cs[r], wim = ga * sn[r];
                wf[(size_t)(2 * t) * ld + 2 * p] = (float)wr;                    // re <- re
                wf[(size_t)(2 * t + 1) * ld + 2 * p] = (float)wim;               // im <- re
                wf[(size_t)(2 * t) * ld + 2 * p + 1] = (float)(-conj * wim);     // re <- im
                wf[(size_t)(2 * t + 1) * ld + 2 * p + 1] = (float)(conj * wr);   // im <- im
                // synthesis: rows are coefficients t, columns spectrum positions p:
                // w = gs * e^{-i 2 pi q t / n}
                const double vr = gs * cs[r], vi = -gs * sn[r];
                wi[(size_t)(2 * p) * ld + 2 * t] = (float)vr;                    // re <- re
                wi[(size_t)(2 * p + 1) * ld + 2 * t] = (float)vi;                // im <- re
                wi[(size_t)(2 * p) * ld + 2 * t + 1] = (float)(-vi);             // re <- im
                wi[(size_t)(2 * p + 1) * ld + 2 * t + 1] = (float)vr;            // im <- im
            }
        }
    }
}

// spectrum coverage (which bands add into bin k), as a CSR over the bins: the gather of the rocFFT path
static void build_coverage(const xsq_plan* P, std::vector<int>& cov_ptr, std::vector<int>& cov_band) {
    cov_ptr.assign(P->nbins + 1, 0);
    std::vector<std::vector<int>> cov(P->nbins);
    for (int j = 0; j < P->nbands; ++j)
        for (int p = 0; p < P->bands[j].Lg; ++p) {
            const int k = P->bands[j].bin0 + p;
            if (k >= 0 && k <= P->L / 2) cov[k].push_back(j);
        }
    for (int k = 0; k < P->nbins; ++k) {
        cov_ptr[k + 1] = cov_ptr[k] + (int)cov[k].size();
        cov_band.insert(cov_band.end(), cov[k].begin(), cov[k].end());
    }
}

// Tables of the hand-written slice FFT (L == FFT_L): the twiddles T, and the phase-ordered entry table of the inverse gather
// -- bands j with j % 4 == ph are laid out back to back; .ent of every band and phase_begin are set here.  False when bands
// of one phase overlap inside [0, L/2]: the gather then has no table (and the plan runs rocFFT).
static bool build_slice_fft_tables(xsq_plan* P, std::vector<float2>& T, std::vector<int>& tgt, std::vector<unsigned short>& tgt16) {
    const int L = P->L, nbands = P->nbands;
    auto W = [&](int64_t j) {   // exp(-2 pi i j / L), argument reduced exactly
        j %= L;
        return make_float2((float)std::cos(PI2 * j / L), (float)(-std::sin(PI2 * j / L)));
    };
    for (int k1 = 0; k1 < FFT_R1; ++k1)
        for (int m = 0; m < FFT_M1; ++m) T.push_back(W(2 * (int64_t)k1 * m));
    for (int k2 = 0; k2 < FFT_R2; ++k2)
        for (int n3 = 0; n3 < FFT_R3; ++n3) T.push_back(W(2 * (int64_t)FFT_R1 * n3 * k2));
    for (int k = 0; k <= FFT_N; ++k) T.push_back(W(k));
    bool ok = true;
    for (int ph = 0; ph < 4; ++ph) {
        P->phase_begin[ph] = (int)tgt.size();
        int last_end = -(1 << 30);
        for (int j = ph; j < nbands; j += 4) {
            BandDev& b = P->bands[j];
            b.ent = (int)tgt.size();
            const int lo = b.bin0 < 0 ? 0 : b.bin0;
            if (lo < last_end) ok = false;
            last_end = b.bin0 + b.Lg > L / 2 + 1 ? L / 2 + 1 : b.bin0 + b.Lg;
            for (int q = 0; q < b.Lg; ++q) {
                const int k = b.bin0 + q;
                tgt.push_back(k >= 0 && k <= L / 2 ? k : -1);
            }
        }
    }
    P->phase_begin[4] = (int)tgt.size();
    // the same table as 16-bit bins (0xFFFF = none) + pad entries: pairs of entries load as one dword
    tgt16.assign(tgt.size() + 2, 0xFFFFu);
    for (size_t i = 0; i < tgt.size(); ++i) tgt16[i] = tgt[i] >= 0 ? (unsigned short)tgt[i] : 0xFFFFu;
    return ok;
}

// Tables of the radix-4 band kernels (band_dft4.h, band_dft4s.h) over the bands with Lg >= the split point; the other bands
// go to bands4_small (the dense engine, gemm_tile.h; the analysis of those above LONG_LG to k_band_fwd_long) and get their
// flag in is_short.
// `commit` false: only the pools are wanted (the adjoint's windows over the band split the plan already has) -- the plan stays as it is.
static void build_radix4_tables(xsq_plan* P, const PlanArgs& A, std::vector<Band4Dev>& b4, std::vector<float>& pf, std::vector<float>& pi,
                                std::vector<char>& is_short, bool commit = true) {
    const int d4_min_lg = switches().d4_min_lg;
    is_short.assign(A.nbands, 0);
    std::map<int, int64_t> doff, twoff, coff;
    auto alloc2 = [&](size_t n) { size_t o = pf.size(); pf.resize(o + n, 0.f); pi.resize(o + n, 0.f); return (int64_t)o; };    // analysis / synthesis pools
    for (int j = 0; j < A.nbands; ++j) {
        const BandDev& b = P->bands[j];
        if (P->on_fft[j]) continue;                 // (band_fft.h: neither engine's)
        if (b.Lg < d4_min_lg || b.Lg > 4 * D4_MPAD) { if (commit) P->bands4_small.push_back(j); is_short[j] = 1; continue; }
        const int n = b.Lg, m = n / 4;
        Band4Dev d;
        memset(&d, 0, sizeof(d));
        d.Lg = n; d.m = m; d.bin0 = b.bin0; d.f = b.f; d.F = b.F; d.ent = b.ent; d.cum = b.cum; d.jband = j;
        d.ldd = (int)round_up(2 * m, 16);
        if (!doff.count(m)) {       // Dt[n' = (k, ro)][kk = (t1, ri)] of exp(-+2 pi i k t1 / m)
            const int64_t o = alloc2((size_t)round_up(2 * m, 64) * d.ldd);
            doff[m] = o;
            for (int k = 0; k < m; ++k)
                for (int t1 = 0; t1 < m; ++t1) {
                    const int r = (int)(((int64_t)k * t1) % m);
                    const double cr = std::cos(PI2 * r / m), si = std::sin(PI2 * r / m);
                    for (int dir = 0; dir < 2; ++dir) {       // 0: analysis e^{+}, 1: synthesis e^{-}
                        std::vector<float>& pool = dir ? pi : pf;
                        const double dre = cr, dim = dir ? -si : si;
                        pool[o + (size_t)(2 * k) * d.ldd + 2 * t1] = (float)dre;
                        pool[o + (size_t)(2 * k) * d.ldd + 2 * t1 + 1] = (float)(-dim);
                        pool[o + (size_t)(2 * k + 1) * d.ldd + 2 * t1] = (float)dim;
                        pool[o + (size_t)(2 * k + 1) * d.ldd + 2 * t1 + 1] = (float)dre;
                    }
                }
        }
        d.d_off = doff[m];
        d.K2 = m / 2 + 1; d.ldc = (int)round_up(d.K2, 8);
        if (!coff.count(m)) {       // band_dft4s.h: Ct[k][n] = cos(2 pi n k / m), St[k][n] = sin(..) with the direction's sign
            const size_t csz = (size_t)round_up(d.K2, 16) * d.ldc;
            const int64_t o = alloc2(2 * csz);
            coff[m] = o;
            for (int k = 0; k < d.K2; ++k)
                for (int nn = 0; nn < d.K2; ++nn) {
                    const int r = (int)(((int64_t)k * nn) % m);
                    const double cr = std::cos(PI2 * r / m), si = (nn == 0 || 2 * nn == m) ? 0.0 : std::sin(PI2 * r / m);
                    pf[o + (size_t)k * d.ldc + nn] = (float)cr;
                    pi[o + (size_t)k * d.ldc + nn] = (float)cr;
                    pf[o + csz + (size_t)k * d.ldc + nn] = (float)(-si);     // analysis e^{+}: X[k] = P + i Q = P - i Q'
                    pi[o + csz + (size_t)k * d.ldc + nn] = (float)si;        // synthesis e^{-}: X[k] = P - i Q
                }
        }
        d.c_off = coff[m];
        if (!twoff.count(n)) {      // twiddles w^(r t1), r = 1..3: [3][round_up(m, 8)] complex
            const int mpad = (m + 7) & ~7;
            const int64_t o = alloc2((size_t)3 * mpad * 2);
            twoff[n] = o;
            for (int r = 1; r <= 3; ++r)
                for (int t1 = 0; t1 < m; ++t1) {
                    const int e = (r * t1) % n;
                    const double cr = std::cos(PI2 * e / n), si = std::sin(PI2 * e / n);
                    pf[o + 2 * ((size_t)(r - 1) * mpad + t1)] = (float)cr;
                    pf[o + 2 * ((size_t)(r - 1) * mpad + t1) + 1] = (float)si;
                    pi[o + 2 * ((size_t)(r - 1) * mpad + t1)] = (float)cr;
                    pi[o + 2 * ((size_t)(r - 1) * mpad + t1) + 1] = (float)(-si);
                }
        }
        d.tw_off = twoff[n];
        d.win_off = alloc2((size_t)round_up(n, 4));
        for (int q = 0; q < n; ++q) {
            pf[d.win_off + q] = (float)A.analysis_window(j, q);
            pi[d.win_off + q] = (float)A.synthesis_window(j, q);
        }
        b4.push_back(d);
        if (!commit) continue;
        P->bands4_m.push_back(m);
        P->d4_max_block = std::max<int64_t>(P->d4_max_block, (int64_t)b.F * b.Lg);
    }
    if (!commit) return;
    P->nbands4 = (int)b4.size();
    P->bands4_host.assign(reinterpret_cast<const unsigned char*>(b4.data()),
                          reinterpret_cast<const unsigned char*>(b4.data()) + b4.size() * sizeof(Band4Dev));
}

// Schedule of the short bands inside k_slice_irfft (slice_fft.h: ShortSched).  Eligible: every band the radix-4 kernel does
// not take has Lg = 4m with 4 <= m <= 15 and lies below the scratch area, the scratch area fits above it, every short band of
// a gather phase precedes every long one, and the work fits the kernel's register arrays.  False: no schedule (the short
// bands stay on the dense engine).
struct ShortTables {
    std::vector<ShortItem1> item1;
    std::vector<float2> tw1;
    std::vector<int> codes, stgt;
    std::vector<float> swd;
    int nent = 0;
};
static bool build_short_schedule(xsq_plan* P, const PlanArgs& A, const std::vector<char>& is_short, ShortTables& H) {
    const int L = A.L, nbands = A.nbands;
    bool ok = true;
    int nent = 0, maxbin = 0;
    for (int j : P->bands4_small) {
        const BandDev& b = P->bands[j];
        if (b.Lg % 4 != 0 || b.Lg < 16 || b.Lg > 60) ok = false;
        nent += b.Lg;
        maxbin = std::max(maxbin, b.bin0 + b.Lg);
    }
    if (maxbin >= SHORT_SCRATCH0 || SHORT_SCRATCH0 + nent > FFT_N + 1) ok = false;
    if (!ok) return false;
    std::vector<std::pair<int, int>> item2;     // (m, code)
    H.nent = nent;
    H.stgt.assign((size_t)nent, -1);
    H.swd.assign((size_t)nent, 0.f);
    int sc = 0;
    for (int ph = 0; ph < 4; ++ph) {
        P->short_begin[ph] = sc;
        for (int j : P->bands4_small) {
            if (j % 4 != ph) continue;
            const BandDev& b = P->bands[j];
            const int n = b.Lg, m = n / 4;
            for (int t1 = 0; t1 < m; ++t1) {
                H.item1.push_back(ShortItem1{(int)b.cum, b.F, b.f, n, t1, sc});
                for (int r = 1; r <= 3; ++r) {
                    const int e = (r * t1) % n;
                    H.tw1.push_back(make_float2((float)std::cos(PI2 * e / n), (float)(-std::sin(PI2 * e / n))));
                }
            }
            for (int r = 0; r < 4; ++r) {
                item2.push_back({m, ((sc + r * m) << 4) | m});
                for (int k = 0; k < m; ++k) {
                    const int q = 4 * k + r;
                    const int bin = b.bin0 + (q + n / 2) % n;
                    H.stgt[sc + r * m + k] = (bin >= 0 && bin <= L / 2) ? bin : -1;
                    H.swd[sc + r * m + k] = (float)A.synthesis_window(j, q);
                }
            }
            sc += n;
        }
    }
    P->short_begin[4] = sc;
    std::stable_sort(item2.begin(), item2.end(), [](const std::pair<int, int>& a, const std::pair<int, int>& b) { return a.first < b.first; });
    for (auto& it : item2) H.codes.push_back(it.second);
    // the gather of the long bands starts behind the short ones of each phase (bands of a phase are in band order)
    for (int ph = 0; ph < 4; ++ph) {
        int lo = P->phase_begin[ph + 1];
        for (int j = ph; j < nbands; j += 4)
            if (!is_short[j]) { lo = P->bands[j].ent; break; }
        P->phase_long[ph] = lo;
        // every short band of the phase must precede every long one, or the split gather would skip entries
        for (int j = ph; j < nbands; j += 4)
            if (is_short[j] && P->bands[j].ent >= lo) ok = false;
    }
    if (!(ok && H.item1.size() <= SHORT_MAX_BUTTERFLIES && H.codes.size() <= SHORT_MAX_DFTS && sc <= nent)) return false;
    for (int ph = 0; ph < 4; ++ph)
        if (P->short_begin[ph + 1] - P->short_begin[ph] > SHORT_MAX_PHASE_ENTRIES) return false;
    return true;
}

// Tables of the FFT band engine (band_fft.h) over the bands of on_fft: one pool per direction (pf analysis, pi synthesis), both
// laid out alike, so one LongBandDev table serves both and the adjoints' pools (`commit` false: only the pools are wanted, the
// plan stays as it is).  Everything is formed in double and rounded once.
static void build_long_tables(xsq_plan* P, const PlanArgs& A, std::vector<LongBandDev>& lb, std::vector<float>& pf, std::vector<float>& pi,
                              bool commit = true) {
    auto alloc2 = [&](size_t n) { size_t o = pf.size(); n = (size_t)round_up((int64_t)n, 4); pf.resize(o + n, 0.f); pi.resize(o + n, 0.f); return (int64_t)o; };
    const auto put = [](std::vector<float>& pool, int64_t o, size_t i, double re, double im) { pool[o + 2 * i] = (float)re; pool[o + 2 * i + 1] = (float)im; };
    std::map<int, int64_t> twoff, choff;
    std::vector<int> order;
    for (int j = 0; j < A.nbands; ++j) if (P->on_fft[j]) order.push_back(j);
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return A.Lg[x] > A.Lg[y]; });     // classes of N: largest first
    for (int j : order) {
        const BandDev& b = P->bands[j];
        const int n = b.Lg, m = n / 4;
        int N = 8;
        while (N < 2 * m - 1) N *= 2;
        LongBandDev d;
        memset(&d, 0, sizeof(d));
        d.Lg = n; d.m = m; d.N = N; d.bin0 = b.bin0; d.f = b.f; d.F = b.F; d.jband = j; d.cum = b.cum;
        if (!twoff.count(N)) {          // e^{-2 pi i k / N}, k < N / 2: both directions' FFT pair
            const int64_t o = twoff[N] = alloc2((size_t)N);
            for (int k = 0; k < N / 2; ++k) { put(pf, o, k, std::cos(PI2 * k / N), -std::sin(PI2 * k / N)); put(pi, o, k, std::cos(PI2 * k / N), -std::sin(PI2 * k / N)); }
        }
        d.tw_off = twoff[N];
        // the chirp c[j] = e^{+ pi i j^2 / m} of the analysis (the synthesis': its conjugate), j^2 reduced mod 2 m
        std::vector<double> cr(m), ci(m);
        for (int i = 0; i < m; ++i) { const int64_t e = ((int64_t)i * i) % (2 * m); cr[i] = std::cos(PI2 * e / (2.0 * m)); ci[i] = std::sin(PI2 * e / (2.0 * m)); }
        if (!choff.count(m)) {          // FFT_N of conj(c) on -(m - 1) .. m - 1 (cyclic), over N, in bit-reversed order
            const int64_t o = choff[m] = alloc2((size_t)2 * N);
            std::vector<double> xr(N, 0.0), xi(N, 0.0);
            for (int i = 0; i < m; ++i) { xr[i] = cr[i]; xi[i] = -ci[i]; if (i) { xr[N - i] = cr[i]; xi[N - i] = -ci[i]; } }
            // decimation in frequency in double, as the kernel's: natural order in, bit-reversed out
            for (int s = N; s >= 2; s >>= 1) {
                const int h = s / 2;
                for (int blk = 0; blk < N; blk += s)
                    for (int i = 0; i < h; ++i) {
                        const double wr = std::cos(PI2 * i / s), wi = -std::sin(PI2 * i / s);
                        const int i0 = blk + i, i1 = i0 + h;
                        const double ur = xr[i0], ui = xi[i0], vr = xr[i1], vi = xi[i1];
                        xr[i0] = ur + vr; xi[i0] = ui + vi;
                        const double dr = ur - vr, di = ui - vi;
                        xr[i1] = dr * wr - di * wi; xi[i1] = dr * wi + di * wr;
                    }
            }
            // the kernel is symmetric (c[-j] = c[j]), so the synthesis' transform is the conjugate of the analysis'
            for (int i = 0; i < N; ++i) { put(pf, o, i, xr[i] / N, xi[i] / N); put(pi, o, i, xr[i] / N, -xi[i] / N); }
        }
        d.chirp_off = choff[m];
        d.pre_off = alloc2((size_t)2 * n);
        d.post_off = alloc2((size_t)2 * n);
        d.win_off = alloc2((size_t)n);
        for (int q = 0; q < n; ++q) {
            const double ga = A.analysis_window(j, q);
            put(pf, d.pre_off, q, ga * cr[q / 4], ga * ci[q / 4]);
            put(pi, d.pre_off, q, cr[q / 4], -ci[q / 4]);
            pi[d.win_off + q] = (float)A.synthesis_window(j, q);
        }
        for (int r = 0; r < 4; ++r)
            for (int k1 = 0; k1 < m; ++k1) {        // c[k1] w^{r k1}: the phase 2 pi (2 (k1^2 mod 2 m) + r k1) / Lg
                const int64_t e = (2 * (((int64_t)k1 * k1) % (2 * m)) + (int64_t)r * k1) % n;
                const double re = std::cos(PI2 * e / n), im = std::sin(PI2 * e / n);
                put(pf, d.post_off, (size_t)r * m + k1, re, im);
                put(pi, d.post_off, (size_t)r * m + k1, re, -im);
            }
        lb.push_back(d);
    }
    if (!commit) return;
    P->nlong = (int)lb.size();
    for (int i = 0; i < P->nlong;) {
        int k = i;
        while (k + 1 < P->nlong && lb[k + 1].N == lb[i].N) ++k;
        P->long_classes.emplace_back(i, k - i + 1, lb[i].N);
        i = k + 1;
    }
}

// one launch per class of N (band_fft.h)
template <bool FWD>
static void launch_band_fft(const xsq_plan* P, const LongArgs& a, int rows, hipStream_t stream) {
    for (const auto& cl : P->long_classes)
        hipLaunchKernelGGL(k_band_fft<FWD>, dim3(rows, std::get<1>(cl)), dim3(LF_NT), (size_t)std::get<2>(cl) * sizeof(float2), stream, a,
                           std::get<0>(cl));
}

// Tables of the mirrored synthesis (dc_twins.h) from Lg, c and gd alone: band j = 1 .. nbands - 2 with 0 < c_j < Lg_j / 2 lands
// on bin q - c_j for c_j <= q < Lg_j / 2 with the weight (-1)^(c_j/2) (-1)^q Lg_j gd_j[Lg_j - q] / L (the inverse slice FFT is
// unnormalised: the 1/L sits in the weights, as in Wi).  Synthesis entries by bin, then band; the transpose's by band, then q,
// with the irfft weight of the bin folded in.
static int build_twin_tables(xsq_plan* P, const PlanArgs& A) {
    std::map<int, std::vector<TwinSrc>> by_bin;
    std::vector<TwinDst> bands;
    std::vector<TwinSrc> asrc;
    std::map<int, int> tw_off;
    std::vector<float2> tw;
    for (int j = 1; j < A.nbands - 1; ++j) {
        const int n = A.Lg[j], cj = A.c[j];
        if (!(cj > 0 && cj < n / 2)) continue;
        if (!tw_off.count(n)) {
            tw_off[n] = (int)tw.size();
            for (int r = 0; r < n; ++r) tw.push_back(make_float2((float)std::cos(PI2 * r / n), (float)std::sin(PI2 * r / n)));
        }
        bands.push_back(TwinDst{j, (int)asrc.size(), n / 2 - cj, tw_off[n]});
        for (int q = cj; q < n / 2; ++q) {
            const int k = q - cj;
            const double w = A.sign(j) * (q % 2 ? -1.0 : 1.0) * n * A.gd[A.g_off[j] + n - q] / A.L;
            by_bin[k].push_back(TwinSrc{j, q + 1, tw_off[n], (float)w});
            asrc.push_back(TwinSrc{k, q + 1, tw_off[n], (float)((k == 0 || k == A.L / 2) ? w : 2.0 * w)});
        }
    }
    std::vector<TwinDst> bins;
    std::vector<TwinSrc> src;
    for (auto& kv : by_bin) {
        bins.push_back(TwinDst{kv.first, (int)src.size(), (int)kv.second.size(), 0});
        src.insert(src.end(), kv.second.begin(), kv.second.end());
    }
    int rc;
    if ((rc = upload(P->d_twin_bins, bins))) return rc;
    if ((rc = upload(P->d_twin_src, src))) return rc;
    if ((rc = upload(P->d_twin_bands, bands))) return rc;
    if ((rc = upload(P->d_twin_asrc, asrc))) return rc;
    if ((rc = upload(P->d_twin_tw, tw))) return rc;
    P->ntwin_bins = (int)bins.size(); P->ntwin_bands = (int)bands.size(); P->ntwins = (int)src.size();
    return XSQ_OK;
}

static int plan_build(xsq_plan* P, int L, int tr, int nbands, const int32_t* Lg, const int32_t* c,
                      const float* g, const double* gd, const float* tw, bool twins, bool long_bands) {
    P->long_bands = long_bands;
    PlanArgs A{L, tr, nbands, Lg, c, g, gd, tw, std::vector<int64_t>(nbands, 0)};
    for (int j = 1; j < nbands; ++j) A.g_off[j] = A.g_off[j - 1] + Lg[j - 1];
    int rc;
    if ((rc = build_band_tables(P, A))) return rc;

    std::vector<float> Wf, Wi;
    build_dense_matrices(P, A, Wf, Wi);
    if ((rc = upload(P->d_Wf, Wf))) return rc;
    P->wf_floats = Wf.size();
    if ((rc = upload(P->d_Wi, Wi))) return rc;

    std::vector<int> cov_ptr, cov_band;
    build_coverage(P, cov_ptr, cov_band);
    if ((rc = upload(P->d_cov_ptr, cov_ptr))) return rc;
    if ((rc = upload(P->d_cov_band, cov_band))) return rc;

    bool phase_table = false;
    if (L == FFT_L) {
        std::vector<float2> T;
        std::vector<int> tgt;
        std::vector<unsigned short> tgt16;
        phase_table = build_slice_fft_tables(P, T, tgt, tgt16);
        if ((rc = upload(P->d_T, T))) return rc;
        if (phase_table) {
            if ((rc = upload(P->d_tgt, tgt))) return rc;
            if ((rc = upload(P->d_tgt16, tgt16))) return rc;
        }
    }
    // the band table, once .ent is known.  The kernels read .ent only beside a phase table (lds_fft): without one the device
    // copy carries 0 there, the host copy and the Band4Dev entries the offsets.
    {
        std::vector<BandDev> dev = P->bands;
        if (!phase_table) for (BandDev& b : dev) b.ent = 0;
        if ((rc = upload(P->d_bands, dev))) return rc;
    }

    std::vector<char> is_short;
    {
        std::vector<Band4Dev> b4;
        std::vector<float> pf, pi;
        build_radix4_tables(P, A, b4, pf, pi, is_short);
        if (P->nbands4) {
            if ((rc = upload(P->d_bands4, b4))) return rc;
            if ((rc = upload(P->d_pool4f, pf))) return rc;
            P->pool4_floats = pf.size();
            if ((rc = upload(P->d_pool4i, pi))) return rc;
        }
    }
    {
        std::vector<LongBandDev> lb;
        std::vector<float> pf, pi;
        build_long_tables(P, A, lb, pf, pi);
        if (P->nlong) {
            if ((rc = upload(P->d_long, lb))) return rc;
            if ((rc = upload(P->d_poolLf, pf))) return rc;
            P->poolL_floats = pf.size();
            if ((rc = upload(P->d_poolLi, pi))) return rc;
        }
    }
    if ((rc = upload(P->d_tw, tw, (size_t)L))) return rc;
    // what the adjoint tables are made from on first use (adjoint_tables)
    P->h_Lg.assign(Lg, Lg + nbands); P->h_c.assign(c, c + nbands);
    P->h_gd.assign(gd, gd + A.g_off[nbands - 1] + Lg[nbands - 1]);
    P->h_g.assign(g, g + A.g_off[nbands - 1] + Lg[nbands - 1]);

    // (needs the LDS slice FFT's gather table, and both kinds of band)
    ShortTables H;
    if (P->d_tgt != nullptr && P->nbands4 > 0 && !P->bands4_small.empty() && build_short_schedule(P, A, is_short, H)) {
        if ((rc = upload(P->d_s_item1, H.item1))) return rc;
        if ((rc = upload(P->d_s_tw1, H.tw1))) return rc;
        if ((rc = upload(P->d_s_item2, H.codes))) return rc;
        if ((rc = upload(P->d_s_tgt, H.stgt))) return rc;
        if ((rc = upload(P->d_s_wd, H.swd))) return rc;
        P->short_n1 = (int)H.item1.size(); P->short_n2 = (int)H.codes.size();
        P->short_nent = H.nent; P->short_sc0 = SHORT_SCRATCH0;
    }
    if (twins && (rc = build_twin_tables(P, A))) return rc;
    return XSQ_OK;
}

// xsq_plan_create (twins false: a plan whose dropped mirrored synthesis is not negligible is refused), xsq_plan_create_twins and
// xsq_plan_create_flags (long_bands: the bands above LONG_LG on the FFT band engine, band_fft.h)
static int plan_create(const char* who, bool twins, bool long_bands, xsq_plan** out, int L, int tr, int nbands, const int32_t* Lg, const int32_t* c,
                       const float* g, const double* gd, const float* tw) {
    XSQ_REQUIRE(out && Lg && c && g && gd && tw, "%s: null argument", who);
    XSQ_REQUIRE(L > 0 && L % 4 == 0 && tr % 2 == 0 && nbands >= 2, "%s: bad L/tr/nbands", who);
    if (!twins) {   // no silently different audio
        std::vector<double> share(nbands);
        int worst = 0;
        if (int rc = xsq_slicqt_dropped_twin_share(L, nbands, Lg, c, gd, share.data(), &worst)) return rc;
        XSQ_REQUIRE(share[worst] < XSQ_TWIN_SHARE_MAX,
                    "xsq_plan_create: band %d (centre bin %d, Lg %d) reaches across DC and the reference's mirrored synthesis of it, "
                    "which this library does not compute, is %.3g of the band's own (limit %.3g): plan refused",
                    worst, (int)c[worst], (int)Lg[worst], share[worst], (double)XSQ_TWIN_SHARE_MAX);
    }
    xsq_plan* P = new xsq_plan();
    const int rc = plan_build(P, L, tr, nbands, Lg, c, g, gd, tw, twins, long_bands);
    if (rc != XSQ_OK) {          // frees whatever was allocated before the failure
        xsq_plan_destroy(P);
        return rc;
    }
    *out = P;
    return XSQ_OK;
}

}  // namespace xsq

using namespace xsq;

extern "C" {

int xsq_abi_version(void) { return XSQ_ABI_VERSION; }

#ifndef XSQ_BUILD_ARCH
#define XSQ_BUILD_ARCH "unknown"
#endif
#ifndef XSQ_BUILD_FLAGS
#define XSQ_BUILD_FLAGS ""
#endif
const char* xsq_build_info(void) { return "arch=" XSQ_BUILD_ARCH "; flags=" XSQ_BUILD_FLAGS "; date=" __DATE__ " " __TIME__; }
const char* xsq_last_error(void) { return g_err; }

int xsq_plan_create(xsq_plan** out, int L, int tr, int nbands, const int32_t* Lg, const int32_t* c,
                    const float* g, const double* gd, const float* tw) {
    return plan_create("xsq_plan_create", false, false, out, L, tr, nbands, Lg, c, g, gd, tw);
}

int xsq_plan_create_twins(xsq_plan** out, int L, int tr, int nbands, const int32_t* Lg, const int32_t* c,
                          const float* g, const double* gd, const float* tw) {
    return plan_create("xsq_plan_create_twins", true, false, out, L, tr, nbands, Lg, c, g, gd, tw);
}

int xsq_plan_create_flags(xsq_plan** out, int L, int tr, int nbands, const int32_t* Lg, const int32_t* c,
                          const float* g, const double* gd, const float* tw, unsigned flags) {
    XSQ_REQUIRE(!(flags & ~(unsigned)(XSQ_PLAN_TWINS | XSQ_PLAN_LONG_BANDS)), "xsq_plan_create_flags: unknown flags 0x%x", flags);
    return plan_create("xsq_plan_create_flags", (flags & XSQ_PLAN_TWINS) != 0, (flags & XSQ_PLAN_LONG_BANDS) != 0, out, L, tr, nbands, Lg, c, g, gd, tw);
}

int xsq_plan_long_band_max(void) { return LF_MAX_LG; }
int xsq_plan_long_band_min(void) { return LONG_LG; }
int xsq_plan_num_long_bands(const xsq_plan* P) { return P ? P->nlong : XSQ_ERR_ARG; }

int xsq_plan_num_twins(const xsq_plan* P) { return P ? P->ntwins : XSQ_ERR_ARG; }

int xsq_plan_destroy(xsq_plan* P) {
    if (!P) return XSQ_OK;
    for (auto& kv : P->fft) {
        if (kv.second.info) rocfft_execution_info_destroy(kv.second.info);
        if (kv.second.plan) rocfft_plan_destroy(kv.second.plan);
    }
    for (auto& kv : P->tiles) (void)hipFree(kv.second.d_tiles);
    (void)hipFree(P->d_bands4); (void)hipFree(P->d_pool4f); (void)hipFree(P->d_pool4i);
    (void)hipFree(P->d_T); (void)hipFree(P->d_tgt); (void)hipFree(P->d_tgt16); (void)hipFree(P->d_tw); (void)hipFree(P->d_Wf); (void)hipFree(P->d_Wi); (void)hipFree(P->d_bands);
    (void)hipFree(P->d_cov_ptr); (void)hipFree(P->d_cov_band);
    (void)hipFree(P->d_adj_tw); (void)hipFree(P->d_adj_Wf); (void)hipFree(P->d_adj_pool4f);
    (void)hipFree(P->d_fadj_Wi); (void)hipFree(P->d_fadj_pool4i); (void)hipFree(P->d_fold_dst); (void)hipFree(P->d_fold_src);
    (void)hipFree(P->d_fold_inl_dst); (void)hipFree(P->d_fold_inl_src);
    (void)hipFree(P->d_twin_bins); (void)hipFree(P->d_twin_src); (void)hipFree(P->d_twin_bands); (void)hipFree(P->d_twin_asrc); (void)hipFree(P->d_twin_tw);
    (void)hipFree(P->d_long); (void)hipFree(P->d_poolLf); (void)hipFree(P->d_poolLi); (void)hipFree(P->d_adj_poolLf); (void)hipFree(P->d_fadj_poolLi);
    (void)hipFree(P->d_s_item1); (void)hipFree(P->d_s_tw1); (void)hipFree(P->d_s_item2); (void)hipFree(P->d_s_tgt); (void)hipFree(P->d_s_wd);
    delete P;
    return XSQ_OK;
}

int xsq_plan_num_blocks(const xsq_plan* P) { return P ? P->nblocks : XSQ_ERR_ARG; }

int xsq_plan_set_band_radix4(xsq_plan* P, int on) {
    XSQ_REQUIRE(P, "xsq_plan_set_band_radix4: null plan");
    P->band_radix4 = on ? 1 : 0;
    return XSQ_OK;
}

#if XSQ_D4_STAMP
extern "C" int xsq_debug_d4_stamps(unsigned long long* host, int tiles) {
    XSQ_HIP(hipDeviceSynchronize());
    XSQ_HIP(hipMemcpyFromSymbol(host, HIP_SYMBOL(g_d4_stamps), (size_t)(tiles < D4_STAMP_TILES ? tiles : D4_STAMP_TILES) * 64));
    return XSQ_OK;
}
#endif
#if XSQ_FFT_STAMP
// diagnostic builds only (not declared in the public header): copies the phase stamps of the last inverse launches
extern "C" int xsq_debug_fft_stamps(unsigned long long* host, int rows) {
    XSQ_HIP(hipDeviceSynchronize());
    XSQ_HIP(hipMemcpyFromSymbol(host, HIP_SYMBOL(g_fft_stamps), (size_t)(rows < FFT_STAMP_ROWS ? rows : FFT_STAMP_ROWS) * 64));
    return XSQ_OK;
}
#endif

int xsq_plan_set_packed_fft(xsq_plan* P, int on) {
    XSQ_REQUIRE(P, "xsq_plan_set_packed_fft: null plan");
#if !XSQ_PACKED_FFT_KERNELS
    // The product library does not contain the packed-fp32 transform: next to v_mfma_f32_16x16x32_bf16 waves of another
    // stream it returned wrong values (tools/probe/pk_mfma_hazard.hip, cause below the ISA), no guard at this level can
    // see what other streams or a later precision switch put beside it, and it measured no faster.
    XSQ_REQUIRE(!on, "xsq_plan_set_packed_fft: this library is built without the packed-fp32 slice FFT kernels "
                "(diagnostic build: make PACKED_FFT=1)");
#endif
    P->packed_fft = on ? 1 : 0;
    return XSQ_OK;
}

int xsq_plan_set_short_inline(xsq_plan* P, int on) {
    XSQ_REQUIRE(P, "xsq_plan_set_short_inline: null plan");
    P->short_inline = on ? 1 : 0;
    return XSQ_OK;
}

int xsq_plan_set_fft_backend(xsq_plan* P, int backend) {
    XSQ_REQUIRE(P && (backend == 0 || backend == 1), "xsq_plan_set_fft_backend: backend must be 0 (auto) or 1 (rocFFT)");
    P->fft_backend = backend;
    return XSQ_OK;
}

int xsq_plan_block_table(const xsq_plan* P, int64_t* table) {
    XSQ_REQUIRE(P && table, "xsq_plan_block_table: null argument");
    for (int b = 0; b < P->nblocks; ++b) {
        table[4 * b + 0] = P->blocks[b].first_band;
        table[4 * b + 1] = P->blocks[b].F;
        table[4 * b + 2] = P->blocks[b].T;
        table[4 * b + 3] = P->blocks[b].cum;
    }
    return XSQ_OK;
}

int64_t xsq_plan_coefs_per_slice(const xsq_plan* P) { return P ? P->sumFT : XSQ_ERR_ARG; }

int xsq_plan_num_slices(const xsq_plan* P, int64_t n) {
    if (!P || n <= 0) return XSQ_ERR_ARG;
    const int64_t nb = (n + P->h - 1) / P->h;
    return (int)((nb + 1) / 2 + 1);
}

// workspace: seg | U | fft work
size_t xsq_slicqt_forward_workspace(xsq_plan* P, int BC, int64_t n) {
    if (!P || BC <= 0 || n <= 0) return 0;
    const size_t rows = (size_t)BC * xsq_plan_num_slices(P, n);
    FftPlan f;
    if (!lds_fft(P) && get_fft(P, 0, (int)rows, &f)) return 0;
    return al256(rows * P->L * 4) + al256(rows * P->nbins * 8) + al256(f.work_bytes) + 256;
}

int xsq_slicqt_forward(xsq_plan* P, const float* x, int BC, int64_t n, float* coef, void* ws,
                       size_t ws_bytes, void* stream_) {
    return xsq_slicqt_forward_xin(P, x, BC, n, coef, nullptr, nullptr, nullptr, 0, ws, ws_bytes, stream_);
}

int xsq_slicqt_forward_xin(xsq_plan* P, const float* x, int BC, int64_t n, float* coef, float* xin, const float* mean,
                           const float* scale, int split, void* ws, size_t ws_bytes, void* stream_) {
    return xsq_slicqt_forward_rows(P, x, nullptr, BC, n, n, coef, xin, mean, scale, split, ws, ws_bytes, stream_);
}

int xsq_slicqt_forward_rows(xsq_plan* P, const float* x, const int64_t* x_rows, int BC, int64_t n, int64_t n_pad, float* coef,
                            float* xin, const float* mean, const float* scale, int split, void* ws, size_t ws_bytes,
                            void* stream_) {
    XSQ_REQUIRE(x, "xsq_slicqt_forward: null argument");
    return xsq_slicqt_forward_rows_indirect(P, x, nullptr, x_rows, BC, n, n_pad, coef, xin, mean, scale, split, ws, ws_bytes, stream_);
}

// S slices per channel from absolute slice s0 on; ring > 0: x is the ring of a streaming session (k_slice_rfft, RING)
struct RingNew { const float* x; int64_t first, stride; };       // the samples from `first` on, not yet in the ring (row bc at x + bc * stride)
// the window-dependent tables of the analysis: the plan's own (null) or the adjoint's (adjoint_tables)
struct AnalysisTables { const float *tw, *Wf, *pool4f, *poolLf; };
static int forward_impl(xsq_plan* P, const float* x, const float* const* x_slot, const int64_t* x_rows, int BC, int64_t n, int S, int64_t s0,
                        int ring, float* coef, float* xin, const float* mean, const float* scale, int split, void* ws, size_t ws_bytes,
                        void* stream_, RingNew fresh = RingNew{nullptr, 0, 0}, const AnalysisTables* adj = nullptr);

int xsq_slicqt_forward_rows_indirect(xsq_plan* P, const float* x, const float* const* x_slot, const int64_t* x_rows, int BC, int64_t n,
                                     int64_t n_pad, float* coef, float* xin, const float* mean, const float* scale, int split,
                                     void* ws, size_t ws_bytes, void* stream_) {
    XSQ_REQUIRE(P && (x || x_slot) && coef && ws, "xsq_slicqt_forward: null argument");
    XSQ_REQUIRE(BC > 0 && n > 0 && n_pad >= n, "xsq_slicqt_forward: BC=%d n=%lld n_pad=%lld", BC, (long long)n, (long long)n_pad);
    // the kernels read zeros outside [0, n): padding is a slice count
    return forward_impl(P, x, x_slot, x_rows, BC, n, xsq_plan_num_slices(P, n_pad), 0, 0, coef, xin, mean, scale, split, ws, ws_bytes, stream_);
}

int xsq_slicqt_forward_ring(xsq_plan* P, float* ring, int ring_len, int BC, int64_t first_slice, int S, int64_t n, const float* x_new,
                            int64_t new_stride, int64_t new_count, float* coef, float* xin, const float* mean, const float* scale, int split,
                            void* ws, size_t ws_bytes, void* stream_) {
    XSQ_REQUIRE(P && ring && coef && ws, "xsq_slicqt_forward_ring: null argument");
    XSQ_REQUIRE(new_count >= 0 && new_count <= n && (new_count == 0 || (x_new && new_stride >= new_count)),
                "xsq_slicqt_forward_ring: %lld new samples of %lld, row stride %lld", (long long)new_count, (long long)n, (long long)new_stride);
    // every new sample lies in the second half of one slice of the call, which stores it to the ring
    XSQ_REQUIRE(new_count == 0 || ((n - new_count) / (2 * P->h) >= first_slice && (n - 1) / (2 * P->h) < first_slice + S),
                "xsq_slicqt_forward_ring: the new samples [%lld, %lld) are not covered by the second halves of the slices [%lld, %lld)",
                (long long)(n - new_count), (long long)n, (long long)first_slice, (long long)(first_slice + S));
    XSQ_REQUIRE(BC > 0 && S >= 2 && first_slice >= 0 && n > 0, "xsq_slicqt_forward_ring: BC=%d S=%d first_slice=%lld n=%lld", BC, S,
                (long long)first_slice, (long long)n);
    // every sample a row reads is one of the last ring_len fed, and a slice wraps at most once
    XSQ_REQUIRE(ring_len > P->L && (2 * (first_slice + S - 1) + 2) * P->h - std::max<int64_t>(0, (2 * first_slice - 2) * P->h) <= ring_len,
                "xsq_slicqt_forward_ring: %d slices of %d samples do not fit a ring of %d", S, P->L, ring_len);
    XSQ_REQUIRE(first_slice + S < (1ll << 40), "xsq_slicqt_forward_ring: slice index %lld", (long long)first_slice);
    return forward_impl(P, ring, nullptr, nullptr, BC, n, S, first_slice, ring_len, coef, xin, mean, scale, split, ws, ws_bytes, stream_,
                        RingNew{x_new, n - new_count, new_stride});
}

static int forward_impl(xsq_plan* P, const float* x, const float* const* x_slot, const int64_t* x_rows, int BC, int64_t n, int S, int64_t s0,
                        int ring, float* coef, float* xin, const float* mean, const float* scale, int split, void* ws, size_t ws_bytes,
                        void* stream_, RingNew fresh, const AnalysisTables* adj) {
    XSQ_REQUIRE(!xin || (mean && scale), "xsq_slicqt_forward_xin: xin needs the mean / scale tables");
    const float* d_tw = adj ? adj->tw : P->d_tw;
    const float* d_Wf = adj ? adj->Wf : P->d_Wf;
    const float* d_pool4f = adj ? adj->pool4f : P->d_pool4f;
    const float* d_poolLf = adj ? adj->poolLf : P->d_poolLf;
    hipStream_t stream = (hipStream_t)stream_;
    const int rows = BC * S;
    XSQ_REQUIRE(S >= 2, "xsq_slicqt_forward: signal too short");
    XSQ_REQUIRE((int64_t)BC * S <= 65535, "xsq_slicqt_forward: BC*S=%lld rows exceed one launch", (long long)BC * S);
    // band_dft4.h addresses the slice spectra and the arena through 32-bit float offsets
    XSQ_REQUIRE((int64_t)2 * BC * S * (P->sumFT > P->nbins ? P->sumFT : P->nbins) < (1ll << 31),
                "xsq_slicqt_forward: BC*S=%lld rows exceed 2^31 floats of coefficients; split the call", (long long)BC * S);
    if (int rcg = d4_ranges_ok(P, (int64_t)BC * S, "xsq_slicqt_forward")) return rcg;
    FftPlan f;
    int rc = lds_fft(P) ? XSQ_OK : get_fft(P, 0, rows, &f);
    if (rc) return rc;
    char* w = (char*)ws;
    float* seg = (float*)w; w += al256((size_t)rows * P->L * 4);
    float* U = (float*)w;   w += al256((size_t)rows * P->nbins * 8);
    void* fwork = w;
    if ((size_t)(w - (char*)ws) + f.work_bytes > ws_bytes) {
        set_error("xsq_slicqt_forward: workspace too small (%zu needed, %zu given)",
                  (size_t)(w - (char*)ws) + f.work_bytes, ws_bytes);
        return XSQ_ERR_WORKSPACE;
    }
    if (lds_fft(P)) {
        XSQ_PROF(adj ? "adjoint_slice_rfft" : "slice_rfft", stream);
        auto kernel = k_slice_rfft<512>;
#if XSQ_PACKED_FFT_KERNELS
        if (P->packed_fft) kernel = k_slice_rfft<512, true>;
#endif
        if (ring) kernel = k_slice_rfft<512, false, true>;
        hipLaunchKernelGGL(kernel, dim3(rows), dim3(512), 0, stream, x, d_tw, fft_tables(P), (float2*)U, S, n, P->h, x_rows, x_slot, s0, ring,
                           const_cast<float*>(x), fresh.x, fresh.first, fresh.stride);
    } else {
        { XSQ_PROF(adj ? "adjoint_slice_window" : "slice_window", stream);
        hipLaunchKernelGGL(k_slice_window, dim3((P->L + 255) / 256, rows), dim3(256), 0, stream, x, d_tw, seg,
                           S, n, P->L, P->h, x_rows, x_slot, s0, ring, const_cast<float*>(x), fresh.x, fresh.first, fresh.stride); }
        { XSQ_PROF(adj ? "adjoint_rfft_L" : "rfft_L", stream); rc = run_fft(f, seg, U, fwork, stream); }
        if (rc) return rc;
    }
    TileTable tt, tl;
    rc = get_band_tiles(P, rows, &tt, 1);
    if (rc) return rc;
    if ((rc = get_band_tiles(P, rows, &tl, 2))) return rc;
    BandFwdOp op{U, coef, P->d_bands, d_Wf, BC, S, P->nbins, P->L, xin, mean, scale, split};
    if (P->band_radix4 && P->nbands4) {
        Band4Args a4{(const Band4Dev*)P->d_bands4, d_pool4f, U, coef, BC, S, P->nbins, P->L, 0, nullptr, 0, xin, mean, scale, split};
        XSQ_PROF(adj ? "adjoint_band_dft4" : "band_analysis_dft4", stream);
        if ((rc = launch_dft4<true>(P, a4, rows, 0, stream))) return rc;
    }
    if (tt.ntiles) { XSQ_PROF(adj ? "adjoint_band_gemm" : "band_analysis_gemm", stream);
    hipLaunchKernelGGL((grouped_gemm_kernel<BandFwdOp>), dim3(tt.ntiles), dim3(256), 0, stream, op,
                       tt.d_tiles, tt.ntiles); }
    if (tl.ntiles) { XSQ_PROF(adj ? "adjoint_band_long" : "band_analysis_long", stream);
    hipLaunchKernelGGL(k_band_fwd_long, dim3(tl.ntiles), dim3(256), 0, stream, op, (const TileDev*)tl.d_tiles); }
    if (P->nlong) { XSQ_PROF(adj ? "adjoint_band_fft" : "band_analysis_fft", stream);
    launch_band_fft<true>(P, LongArgs{(const LongBandDev*)P->d_long, d_poolLf, U, coef, BC, S, P->nbins, P->L, nullptr, 0, xin, mean, scale, split}, rows, stream); }
    XSQ_HIP(hipGetLastError());
    return XSQ_OK;
}

// ---- adjoint of the inverse transform: gy (BC, length) -> gradient arena ----
// With y = xsq_slicqt_inverse(coef) and gy = dLoss/dy (zero outside [0, length)):
//   gcoef[bc,j,s,:] = (-1)^(c_j/2) IFFT_Lg( a'_j[q] V[bc,s, c_j + sq(q)] ),  V[bc,s,:] = rfft_L( gypad[(2s-2)h : (2s+2)h] )
//   a'_j[q] = [0 <= c_j + sq(q) <= L/2] w_k Lg_j^2 gd_j[q] / L,  w_0 = w_{L/2} = 1, w_k = 2 otherwise
// -- the analysis with a slice window of ones and a' in place of g_j, so it runs on the analysis kernels over tables built
// from a'.  a' is zero on the mirrored entries of the DC and Nyquist bands: what the kernels load there is multiplied away.
int xsq_slicqt_adjoint_window(int L, int nbands, const int32_t* Lg, const int32_t* c, const double* gd, double* out) {
    XSQ_REQUIRE(Lg && c && gd && out, "xsq_slicqt_adjoint_window: null argument");
    XSQ_REQUIRE(L > 0 && L % 4 == 0 && nbands >= 1, "xsq_slicqt_adjoint_window: L=%d nbands=%d", L, nbands);
    int64_t off = 0;
    for (int j = 0; j < nbands; ++j) {
        const int n = Lg[j];
        XSQ_REQUIRE(n > 0 && n % 2 == 0, "xsq_slicqt_adjoint_window: band %d has Lg=%d", j, n);
        for (int q = 0; q < n; ++q) {
            const int k = c[j] + (q < n / 2 ? q : q - n);
            const double w = (k < 0 || k > L / 2) ? 0.0 : ((k == 0 || k == L / 2) ? 1.0 : 2.0);
            out[off + q] = w * (double)n * (double)n * gd[off + q] / (double)L;
        }
        off += n;
    }
    return XSQ_OK;
}

// ---- the part of the reference's inverse that this library does not compute on a plan of xsq_plan_create ----
// (xsq_plan_create_twins computes it: build_twin_tables, dc_twins.h)
// The reference synthesises every band 1 .. nbands-2 a second time through the dual window of its negative-frequency
// mirror (centre L - c_j), from conj(cat(t[1:], flip(t[1:]))) of the band's spectrum t, and keeps bins 0..L/2 of the sum
// (nsgt/nsigtf.py:57-99).  For a band that reaches across DC (0 < c_j < Lg_j/2) that second synthesis lands on the kept
// bins  q - c_j,  c_j <= q < Lg_j/2,  with weight Lg_j gd'_j[q], gd' the mirrored band's dual window = gd_j[Lg_j - q]
// (the windows and the frame diagonal are even).  The kernels drop it.  share[j] = its weight relative to the kept
// synthesis of the band,  sqrt( sum_q gd_j[Lg_j - q]^2 / sum_{0 <= c_j + sq(q) <= L/2} gd_j[q]^2 ),  0 for every other band.
// Host arithmetic, no device.  Returns the band of the largest share in *worst (may be null).
int xsq_slicqt_dropped_twin_share(int L, int nbands, const int32_t* Lg, const int32_t* c, const double* gd, double* share,
                                  int* worst) {
    XSQ_REQUIRE(Lg && c && gd && share, "xsq_slicqt_dropped_twin_share: null argument");
    XSQ_REQUIRE(L > 0 && L % 4 == 0 && nbands >= 1, "xsq_slicqt_dropped_twin_share: L=%d nbands=%d", L, nbands);
    int64_t off = 0;
    int w = 0;
    for (int j = 0; j < nbands; ++j) {
        const int n = Lg[j];
        XSQ_REQUIRE(n > 0 && n % 2 == 0, "xsq_slicqt_dropped_twin_share: band %d has Lg=%d", j, n);
        share[j] = 0.0;
        if (j > 0 && j < nbands - 1 && c[j] > 0 && c[j] < n / 2) {
            double kept = 0.0, dropped = 0.0;
            for (int q = 0; q < n; ++q) {
                const int k = c[j] + (q < n / 2 ? q : q - n);
                if (k >= 0 && k <= L / 2) kept += gd[off + q] * gd[off + q];
            }
            for (int q = c[j]; q < n / 2; ++q) dropped += gd[off + n - q] * gd[off + n - q];
            share[j] = kept > 0.0 ? std::sqrt(dropped / kept) : 1.0;
        }
        if (share[j] > share[w]) w = j;
        off += n;
    }
    if (worst) *worst = w;
    return XSQ_OK;
}

namespace xsq {
// the analysis tables of a', built and uploaded on first use (a synchronous upload: warm a plan up before capturing it)
static int adjoint_tables(xsq_plan* P, AnalysisTables* out) {
    std::lock_guard<std::mutex> lk(P->mu);
    if (!P->adj_built) {
        const int nbands = P->nbands;
        std::vector<double> a(P->h_gd.size());
        if (int rc = xsq_slicqt_adjoint_window(P->L, nbands, P->h_Lg.data(), P->h_c.data(), P->h_gd.data(), a.data())) return rc;
        PlanArgs A{P->L, P->tr, nbands, P->h_Lg.data(), P->h_c.data(), nullptr, P->h_gd.data(), nullptr, std::vector<int64_t>(nbands, 0), a.data()};
        for (int j = 1; j < nbands; ++j) A.g_off[j] = A.g_off[j - 1] + P->h_Lg[j - 1];
        std::vector<float> Wf, Wi, pf, pi;
        build_dense_matrices(P, A, Wf, Wi);
        std::vector<Band4Dev> b4;
        std::vector<char> is_short;
        build_radix4_tables(P, A, b4, pf, pi, is_short, false);
        std::vector<LongBandDev> lb;
        std::vector<float> lf, li;
        build_long_tables(P, A, lb, lf, li, false);
        XSQ_REQUIRE((int)lb.size() == P->nlong && (!P->nlong || lf.size() == P->poolL_floats),
                    "xsq_slicqt_inverse_adjoint: the adjoint's FFT band tables (%zu floats, %zu bands) do not match the plan's (%zu, %d)", lf.size(),
                    lb.size(), P->poolL_floats, P->nlong);
        // The kernels reach both pools through the offsets of the plan's ONE band table (d_bands: w_off; d_bands4: d_off, c_off,
        // tw_off, win_off), so the adjoint's pools must be laid out exactly like the plan's: same builders, same band split (the
        // process switches are read once, switches()), only the window entries differ.  The synthesis halves (Wi, pi) the
        // builders also fill are dropped.  Held here rather than assumed:
        XSQ_REQUIRE(Wf.size() == P->wf_floats && (int)b4.size() == P->nbands4 && (!P->nbands4 || pf.size() == P->pool4_floats),
                    "xsq_slicqt_inverse_adjoint: the adjoint tables (%zu / %zu floats, %zu radix-4 bands) do not match the plan's (%zu / %zu, %d)",
                    Wf.size(), pf.size(), b4.size(), P->wf_floats, P->pool4_floats, P->nbands4);
        const std::vector<float> ones((size_t)P->L, 1.f);
        float *tw = nullptr, *dWf = nullptr, *dpf = nullptr, *dlf = nullptr;
        int rc = upload(tw, ones);
        if (!rc) rc = upload(dWf, Wf);
        if (!rc && P->nbands4) rc = upload(dpf, pf);
        if (!rc && P->nlong) rc = upload(dlf, lf);
        if (rc) { (void)hipFree(tw); (void)hipFree(dWf); (void)hipFree(dpf); (void)hipFree(dlf); return rc; }
        P->d_adj_tw = tw; P->d_adj_Wf = dWf; P->d_adj_pool4f = dpf; P->d_adj_poolLf = dlf;
        P->adj_built = true;
    }
    *out = AnalysisTables{P->d_adj_tw, P->d_adj_Wf, P->d_adj_pool4f, P->d_adj_poolLf};
    return XSQ_OK;
}

// dst[i] += src[i], four floats per thread (arenas are multiples of four floats: T % 4 == 0)
__global__ __launch_bounds__(256) void k_arena_add(float* __restrict__ dst, const float* __restrict__ src, int64_t quads) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= quads) return;
    const float4 a = reinterpret_cast<const float4*>(src)[q];
    float4 d = reinterpret_cast<float4*>(dst)[q];
    d.x += a.x; d.y += a.y; d.z += a.z; d.w += a.w;
    reinterpret_cast<float4*>(dst)[q] = d;
}
}  // namespace xsq

// workspace: [scratch arena when accumulating |] seg | U | fft work
size_t xsq_slicqt_inverse_adjoint_workspace(xsq_plan* P, int BC, int S, int accumulate) {
    if (!P || BC <= 0 || S < 2) return 0;
    const size_t rows = (size_t)BC * S;
    FftPlan f;
    if (!lds_fft(P) && get_fft(P, 0, (int)rows, &f)) return 0;
    return (accumulate ? al256(rows * P->sumFT * 8) : 0) + al256(rows * P->L * 4) + al256(rows * P->nbins * 8) + al256(f.work_bytes) + 256;
}

int xsq_slicqt_inverse_adjoint(xsq_plan* P, const float* gy, int BC, int S, int64_t length, float* gcoef, int accumulate, void* ws,
                               size_t ws_bytes, void* stream_) {
    XSQ_REQUIRE(P && gy && gcoef && ws, "xsq_slicqt_inverse_adjoint: null argument");
    XSQ_REQUIRE(BC > 0 && S >= 2 && length > 0 && length <= (int64_t)2 * S * P->h, "xsq_slicqt_inverse_adjoint: BC=%d S=%d length=%lld", BC, S,
                (long long)length);
    const size_t need = xsq_slicqt_inverse_adjoint_workspace(P, BC, S, accumulate);
    XSQ_REQUIRE(need && need <= ws_bytes, "xsq_slicqt_inverse_adjoint: workspace too small (%zu needed, %zu given)", need, ws_bytes);
    AnalysisTables adj;
    if (int rc = adjoint_tables(P, &adj)) return rc;
    const size_t arena_bytes = (size_t)BC * S * P->sumFT * 8;
    char* w = (char*)ws;
    float* dst = gcoef;
    if (accumulate) { dst = (float*)w; w += al256(arena_bytes); }
    if (int rc = forward_impl(P, gy, nullptr, nullptr, BC, length, S, 0, 0, dst, nullptr, nullptr, nullptr, 0, w, ws_bytes - (size_t)(w - (char*)ws),
                              stream_, RingNew{nullptr, 0, 0}, &adj))
        return rc;
    hipStream_t stream = (hipStream_t)stream_;
    if (P->ntwins) {   // the transpose of the mirrored synthesis (dc_twins.h), from the slice spectra forward_impl left in its workspace (seg | U)
        const float2* V = (const float2*)(w + al256((size_t)BC * S * P->L * 4));
        XSQ_PROF("twin_analysis", stream);
        hipLaunchKernelGGL(k_twin_analysis, dim3(BC * S), dim3(64), 0, stream, V, P->d_bands, (const TwinDst*)P->d_twin_bands,
                           (const TwinSrc*)P->d_twin_asrc, P->d_twin_tw, P->ntwin_bands, dst, BC, S, P->nbins);
        XSQ_HIP(hipGetLastError());
    }
    if (accumulate) {
        const int64_t quads = (int64_t)(arena_bytes / 16);
        XSQ_PROF("adjoint_accumulate", stream);
        hipLaunchKernelGGL(k_arena_add, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, stream, gcoef, dst, quads);
        XSQ_HIP(hipGetLastError());
    }
    return XSQ_OK;
}

// workspace: Z | fr | seg | fft work
size_t xsq_slicqt_inverse_workspace(xsq_plan* P, int BC, int S) {
    if (!P || BC <= 0 || S <= 0) return 0;
    const size_t rows = (size_t)BC * S;
    FftPlan f;
    if (!lds_fft(P) && get_fft(P, 1, (int)rows, &f)) return 0;
    if (lds_fft(P)) return al256(rows * P->sumFT * 8) + 256;        // Z only: spectra and segments stay in LDS
    return al256(rows * P->sumFT * 8) + al256(rows * P->nbins * 8) + al256(rows * P->L * 4) + al256(f.work_bytes) + 256;
}

int xsq_slicqt_inverse(xsq_plan* P, const float* coef, int BC, int S, int64_t length, float* y, void* ws,
                       size_t ws_bytes, void* stream_) {
    return xsq_slicqt_inverse_rows(P, coef, BC, S, length, y, nullptr, ws, ws_bytes, stream_);
}

// carry != nullptr: the S slices are the new ones of a streaming step and `y` takes its blocks (CarryArgs, slice_fft.h)
// adj != nullptr: the adjoint of the forward transform (xsq_slicqt_forward_adjoint) -- the synthesis over the tables of its
// window, the fold of the mirrored entries, and slices multiplied by the slice window before the overlap-add
struct AdjointSynthesis { const float *Wi, *pool4i, *poolLi, *tw; const FoldDst* dst; const FoldSrc* src; int ndst; FoldSched inl; };
static int inverse_impl(xsq_plan* P, const float* coef, const float* mask, int BCx, int BC, int S, int64_t length, float* y,
                        const int64_t* row_offsets, void* ws, size_t ws_bytes, void* stream_, const CarryArgs* carry = nullptr,
                        const AdjointSynthesis* adj = nullptr);

int xsq_slicqt_inverse_rows(xsq_plan* P, const float* coef, int BC, int S, int64_t length, float* y,
                            const int64_t* row_offsets, void* ws, size_t ws_bytes, void* stream_) {
    return inverse_impl(P, coef, nullptr, 0, BC, S, length, y, row_offsets, ws, ws_bytes, stream_);
}

int xsq_slicqt_inverse_masked(xsq_plan* P, const float* masks, const float* mix, int BC, int BCx, int S, int64_t length,
                              float* y, const int64_t* row_offsets, void* ws, size_t ws_bytes, void* stream_) {
    XSQ_REQUIRE(masks && mix, "xsq_slicqt_inverse_masked: null argument");
    XSQ_REQUIRE(BCx > 0 && BC % BCx == 0, "xsq_slicqt_inverse_masked: %d mix channels do not divide %d mask channels", BCx, BC);
    return inverse_impl(P, mix, masks, BCx, BC, S, length, y, row_offsets, ws, ws_bytes, stream_);
}

static int inverse_impl(xsq_plan* P, const float* coef, const float* mask, int BCx, int BC, int S, int64_t length, float* y,
                        const int64_t* row_offsets, void* ws, size_t ws_bytes, void* stream_, const CarryArgs* carry,
                        const AdjointSynthesis* adj) {
    XSQ_REQUIRE(P && coef && y && ws, "xsq_slicqt_inverse: null argument");
    XSQ_REQUIRE(BC > 0 && S >= (carry ? 1 : 2) && length > 0, "xsq_slicqt_inverse: BC=%d S=%d length=%lld", BC, S,
                (long long)length);
    XSQ_REQUIRE(length <= (int64_t)2 * (carry ? carry->nblk : S) * P->h, "xsq_slicqt_inverse: length %lld exceeds the %d slices",
                (long long)length, S);
    XSQ_REQUIRE((int64_t)BC * S <= 65535, "xsq_slicqt_inverse: BC*S=%lld rows exceed one launch", (long long)BC * S);
    // the band kernels carry arena offsets in 32 bits (band_dft4.h: xoff / moff; the mix arena is the smaller one)
    XSQ_REQUIRE((int64_t)2 * BC * S * P->sumFT < (1ll << 31), "xsq_slicqt_inverse: the coefficient arena of BC*S=%lld rows "
                "exceeds 2^31 floats; split the call (fewer stacked chunks)", (long long)BC * S);
    if (int rcg = d4_ranges_ok(P, (int64_t)BC * S, "xsq_slicqt_inverse")) return rcg;
    hipStream_t stream = (hipStream_t)stream_;
    const int rows = BC * S;
    FftPlan f;
    int rc = lds_fft(P) ? XSQ_OK : get_fft(P, 1, rows, &f);
    if (rc) return rc;
    char* w = (char*)ws;
    float* Z = (float*)w;    w += al256((size_t)rows * P->sumFT * 8);
    float2* fr = (float2*)w; if (!lds_fft(P)) w += al256((size_t)rows * P->nbins * 8);
    float* seg = (float*)w;  if (!lds_fft(P)) w += al256((size_t)rows * P->L * 4);
    void* fwork = w;
    if ((size_t)(w - (char*)ws) + f.work_bytes > ws_bytes) {
        set_error("xsq_slicqt_inverse: workspace too small (%zu needed, %zu given)",
                  (size_t)(w - (char*)ws) + f.work_bytes, ws_bytes);
        return XSQ_ERR_WORKSPACE;
    }
    TileTable tt;
    rc = get_band_tiles(P, rows, &tt);
    if (rc) return rc;
    BandInvOp op{coef, Z, P->d_bands, adj ? adj->Wi : P->d_Wi, BC, S, lds_fft(P) ? (int)P->sumFT : 0, mask, BCx};
    if (P->band_radix4 && P->nbands4) {
        Band4Args a4{(const Band4Dev*)P->d_bands4, adj ? adj->pool4i : P->d_pool4i, coef, Z, BC, S, P->nbins, P->L,
                     lds_fft(P) ? (int)P->sumFT : 0, mask, BCx, nullptr, nullptr, nullptr, 0};
        XSQ_PROF(adj ? "fwd_adjoint_band_dft4" : "band_synthesis_dft4", stream);
        if ((rc = launch_dft4<false>(P, a4, rows, mask ? BCx * S : 0, stream))) return rc;
    }
    // short bands: inside k_slice_irfft when the plan allows it, else dense GEMM + Z round trip
    const bool inl = lds_fft(P) && P->band_radix4 && P->short_inline && P->short_n1 > 0 && !carry && !adj;
    if (tt.ntiles && !inl) { XSQ_PROF(adj ? "fwd_adjoint_band_gemm" : "band_synthesis_gemm", stream);
    hipLaunchKernelGGL((grouped_gemm_kernel<BandInvOp>), dim3(tt.ntiles), dim3(256), 0, stream, op,
                       tt.d_tiles, tt.ntiles); }
    if (P->nlong) { XSQ_PROF(adj ? "fwd_adjoint_band_fft" : "band_synthesis_fft", stream);
    launch_band_fft<false>(P, LongArgs{(const LongBandDev*)P->d_long, adj ? adj->poolLi : P->d_poolLi, coef, Z, BC, S, P->nbins, P->L, mask, BCx, nullptr, nullptr, nullptr, 0}, rows, stream); }
    // the fold: inside the hand-written slice FFT (FOLD, slice_fft.h), or a pass over Z in front of the rocFFT path's gather
    if (adj && adj->ndst && !lds_fft(P)) { XSQ_PROF("fwd_adjoint_fold", stream);
    hipLaunchKernelGGL(k_fold_mirrored, dim3(rows), dim3(256), 0, stream, Z, P->d_bands, adj->dst, adj->src, adj->ndst, BC, S); }
    if (lds_fft(P)) {
        // inverse slice FFT with the overlap-add fused in: even slices store, odd slices add (slice_fft.h)
        XSQ_PROF(adj ? "fwd_adjoint_slice_irfft_ola" : "slice_irfft_ola", stream);
        GatherSched G;
        G.tgt = P->d_tgt; G.tgt16 = P->d_tgt16; G.row_len = (int)P->sumFT;
        for (int i = 0; i < 5; ++i) G.begin[i] = P->phase_begin[i];
        for (int i = 0; i < 4; ++i) G.lo[i] = inl ? P->phase_long[i] : P->phase_begin[i];
        ShortSched SS;
        memset(&SS, 0, sizeof(SS));
        if (inl) {
            SS.item1 = (const ShortItem1*)P->d_s_item1; SS.tw1 = (const float2*)P->d_s_tw1; SS.item2 = P->d_s_item2;
            SS.stgt = P->d_s_tgt; SS.swd = P->d_s_wd;
            SS.n1 = P->short_n1; SS.n2 = P->short_n2; SS.nent = P->short_nent; SS.sc0 = P->short_sc0;
            for (int i = 0; i < 5; ++i) SS.begin[i] = P->short_begin[i];
        }
        const ShortIn SI{coef, mask, BC, mask ? BCx : BC};
        // the four-phases-in-flight gather: the default path's, when the 16-bit table exists and every phase fits its registers
        bool fast4 = !inl && G.tgt16 != nullptr;
        for (int ph = 0; ph < 4; ++ph) fast4 = fast4 && (G.begin[ph + 1] - (G.lo[ph] & ~1) <= FAST4_MAX_PHASE_ENTRIES);
        auto kernel = inl ? k_slice_irfft<512, false, true> : fast4 ? k_slice_irfft<512, false, false, true> : k_slice_irfft<512>;
#if XSQ_PACKED_FFT_KERNELS
        if (P->packed_fft && !inl) kernel = fast4 ? k_slice_irfft<512, true, false, true> : k_slice_irfft<512, true>;
#endif
        if (carry) kernel = fast4 ? k_slice_irfft<512, false, false, true, true> : k_slice_irfft<512, false, false, false, true>;
        if (adj) kernel = fast4 ? k_slice_irfft<512, false, false, true, false, true, true> : k_slice_irfft<512, false, false, false, false, true, true>;
        for (int parity = 0; parity < 2; ++parity) {
            const int nsl = (S + 1 - parity) / 2;
            if (!nsl) continue;                   // (a step of one slice has no odd one)
            OlaArgs O{y, row_offsets, S, P->h, parity, length};
            hipLaunchKernelGGL(kernel, dim3(BC * nsl), dim3(512), 0, stream, (const float2*)Z, G, fft_tables(P), O, SS, SI, carry ? *carry : CarryArgs{},
                               adj ? adj->tw : (const float*)nullptr, adj ? adj->inl : FoldSched{});
        }
        XSQ_HIP(hipGetLastError());
        return XSQ_OK;
    } else {
        { XSQ_PROF(adj ? "fwd_adjoint_spectrum_gather" : "spectrum_gather", stream);
        hipLaunchKernelGGL(k_spectrum_gather, dim3((P->nbins + 255) / 256, rows), dim3(256), 0, stream, Z,
                           P->d_bands, P->d_cov_ptr, P->d_cov_band, fr, BC, S, P->nbins); }
        // the mirrored synthesis of the bands across DC (dc_twins.h); not in the adjoint of the analysis, which has no such term
        if (P->ntwins && !adj) { XSQ_PROF("twin_synthesis", stream);
        hipLaunchKernelGGL(k_twin_synthesis, dim3(rows), dim3(64), 0, stream, coef, mask, BCx, P->d_bands, (const TwinDst*)P->d_twin_bins,
                           (const TwinSrc*)P->d_twin_src, P->d_twin_tw, P->ntwin_bins, fr, BC, S, P->nbins); }
        { XSQ_PROF(adj ? "fwd_adjoint_irfft_L" : "irfft_L", stream); rc = run_fft(f, fr, seg, fwork, stream); }
        if (rc) return rc;
    }
    if (adj) {
        XSQ_PROF("fwd_adjoint_overlap_add", stream);
        hipLaunchKernelGGL(k_overlap_add_windowed, dim3((unsigned)((length + 255) / 256), BC), dim3(256), 0, stream, seg, adj->tw, y, S,
                           length, P->L, P->h);
        XSQ_HIP(hipGetLastError());
        return XSQ_OK;
    }
    if (carry) { XSQ_PROF("overlap_add_carry", stream);
    hipLaunchKernelGGL(k_overlap_add_carry, dim3((unsigned)(((carry->nblk + 1) * 2 * P->h + 255) / 256), BC), dim3(256), 0, stream, seg, y,
                       *carry, S, length, P->L, P->h); }
    else { XSQ_PROF("overlap_add", stream);
    hipLaunchKernelGGL(k_overlap_add, dim3((unsigned)((length + 255) / 256), BC), dim3(256), 0, stream, seg, y,
                       row_offsets, S, length, P->L, P->h); }
    XSQ_HIP(hipGetLastError());
    return XSQ_OK;
}

// ---- adjoint of the forward transform: gcoef (gradient arena) -> gx (BC, n) ----
// With coef = xsq_slicqt_forward(x) and G = dLoss/dcoef (real view, arena layout):
//   V[s,j,q] = (-1)^(c_j/2) g_j[q] / Lg_j FFT_Lg( G[s,j,:] )[q],  k = (c_j + sq(q)) mod L
//   fr_s[k] += V[s,j,q] (k <= L/2),  fr_s[L - k] += conj V[s,j,q] (k > L/2: the fold),
//   seg_s = tw . irfft_L( w fr_s ),  w_0 = w_{L/2} = L, w_k = L/2 otherwise,   gx[m] = sum_s seg_s[m + 2h - 2sh]
// -- the synthesis with b_j[q] = g_j[q] / Lg_j w'(bin the entry lands on) in place of gd_j[q] Lg_j / L (w' = w / L: the slice
// transform of the inverse is unnormalised), the fold (k_fold_mirrored) between the band kernels and the gather, and the slice
// window on the way into the overlap-add.  A folded entry lands on a bin strictly inside (0, L/2): its weight is 1/2.
int xsq_slicqt_forward_adjoint_window(int L, int nbands, const int32_t* Lg, const int32_t* c, const float* g, double* out) {
    XSQ_REQUIRE(Lg && c && g && out, "xsq_slicqt_forward_adjoint_window: null argument");
    XSQ_REQUIRE(L > 0 && L % 4 == 0 && nbands >= 1, "xsq_slicqt_forward_adjoint_window: L=%d nbands=%d", L, nbands);
    int64_t off = 0;
    for (int j = 0; j < nbands; ++j) {
        const int n = Lg[j];
        XSQ_REQUIRE(n > 0 && n % 2 == 0 && n <= L / 2 && c[j] >= 0 && c[j] <= L / 2, "xsq_slicqt_forward_adjoint_window: band %d has Lg=%d c=%d",
                    j, n, c[j]);
        for (int q = 0; q < n; ++q) {
            int k = c[j] + (q < n / 2 ? q : q - n);
            if (k < 0) k = -k; else if (k > L / 2) k = L - k;
            const double w = (k == 0 || k == L / 2) ? 1.0 : 0.5;
            out[off + q] = w * (double)g[off + q] / (double)n;
        }
        off += n;
    }
    return XSQ_OK;
}

namespace xsq {
// the synthesis tables of that window and the fold list, built and uploaded on first use (a synchronous upload: warm a plan
// up before capturing it)
static int forward_adjoint_tables(xsq_plan* P, AdjointSynthesis* out) {
    std::lock_guard<std::mutex> lk(P->mu);
    if (!P->fadj_built) {
        const int nbands = P->nbands, L = P->L;
        std::vector<double> b(P->h_g.size());
        if (int rc = xsq_slicqt_forward_adjoint_window(L, nbands, P->h_Lg.data(), P->h_c.data(), P->h_g.data(), b.data())) return rc;
        // (the builders fill both directions: the analysis halves are made from b as well and dropped)
        PlanArgs A{L, P->tr, nbands, P->h_Lg.data(), P->h_c.data(), nullptr, P->h_gd.data(), nullptr, std::vector<int64_t>(nbands, 0), b.data(), b.data()};
        for (int j = 1; j < nbands; ++j) A.g_off[j] = A.g_off[j - 1] + P->h_Lg[j - 1];
        std::vector<float> Wf, Wi, pf, pi;
        build_dense_matrices(P, A, Wf, Wi);
        std::vector<Band4Dev> b4;
        std::vector<char> is_short;
        build_radix4_tables(P, A, b4, pf, pi, is_short, false);
        std::vector<LongBandDev> lb;
        std::vector<float> lf, li;
        build_long_tables(P, A, lb, lf, li, false);
        XSQ_REQUIRE((int)lb.size() == P->nlong && (!P->nlong || li.size() == P->poolL_floats),
                    "xsq_slicqt_forward_adjoint: the adjoint's FFT band tables (%zu floats, %zu bands) do not match the plan's (%zu, %d)", li.size(),
                    lb.size(), P->poolL_floats, P->nlong);
        // same layout as the plan's own pools: the kernels reach them through the plan's ONE band table (see adjoint_tables)
        XSQ_REQUIRE(Wi.size() == P->wf_floats && (int)b4.size() == P->nbands4 && (!P->nbands4 || pi.size() == P->pool4_floats),
                    "xsq_slicqt_forward_adjoint: the adjoint tables (%zu / %zu floats, %zu radix-4 bands) do not match the plan's (%zu / %zu, %d)",
                    Wi.size(), pi.size(), b4.size(), P->wf_floats, P->pool4_floats, P->nbands4);
        // the fold list: every entry whose bin lies outside [0, L/2], onto an entry that lands on the mirrored bin -- of its own
        // band when there is one, else of the first band that covers the bin
        std::map<std::pair<int, int>, std::vector<FoldSrc>> by_dst;
        for (int j = 0; j < nbands; ++j) {
            const BandDev& bj = P->bands[j];
            for (int p = 0; p < bj.Lg; ++p) {
                const int k = bj.bin0 + p;
                if (k >= 0 && k <= L / 2) continue;
                const int m = k < 0 ? -k : L - k;
                int jd = -1;
                if (m >= bj.bin0 && m < bj.bin0 + bj.Lg) jd = j;
                for (int i = 0; jd < 0 && i < nbands; ++i)
                    if (m >= P->bands[i].bin0 && m < P->bands[i].bin0 + P->bands[i].Lg) jd = i;
                XSQ_REQUIRE(jd >= 0 && m >= 0 && m <= L / 2, "xsq_slicqt_forward_adjoint: no band covers bin %d, the mirror of band %d's bin %d", m, j, k);
                by_dst[{jd, m - P->bands[jd].bin0}].push_back(FoldSrc{j, p});
            }
        }
        std::vector<FoldDst> fd;
        std::vector<FoldSrc> fs;
        for (auto& kv : by_dst) {
            fd.push_back(FoldDst{kv.first.first, kv.first.second, (int)fs.size(), (int)kv.second.size()});
            fs.insert(fs.end(), kv.second.begin(), kv.second.end());
        }
        // the same list for the hand-written slice FFT (FoldSched): per mirrored bin, the entries of a row of Z that fold onto it
        std::map<int, std::vector<int>> by_bin;
        if (P->d_tgt)
            for (auto& kv : by_dst)
                for (const FoldSrc& sr : kv.second) by_bin[P->bands[kv.first.first].bin0 + kv.first.second].push_back(P->bands[sr.js].ent + sr.ps);
        std::vector<int4> id;
        std::vector<int> is;
        for (auto& kv : by_bin) { id.push_back(make_int4(kv.first, (int)is.size(), (int)kv.second.size(), 0)); is.insert(is.end(), kv.second.begin(), kv.second.end()); }
        float *dWi = nullptr, *dpi = nullptr, *dli = nullptr;
        void *dd = nullptr, *ds = nullptr, *did = nullptr, *dis = nullptr;
        int rc = upload(dWi, Wi);
        if (!rc && P->nbands4) rc = upload(dpi, pi);
        if (!rc && P->nlong) rc = upload(dli, li);
        if (!rc) rc = upload(dd, fd);
        if (!rc) rc = upload(ds, fs);
        if (!rc) rc = upload(did, id);
        if (!rc) rc = upload(dis, is);
        if (rc) { (void)hipFree(dWi); (void)hipFree(dpi); (void)hipFree(dli); (void)hipFree(dd); (void)hipFree(ds); (void)hipFree(did); (void)hipFree(dis); return rc; }
        P->d_fadj_Wi = dWi; P->d_fadj_pool4i = dpi; P->d_fadj_poolLi = dli; P->d_fold_dst = dd; P->d_fold_src = ds; P->nfold_dst = (int)fd.size();
        P->d_fold_inl_dst = did; P->d_fold_inl_src = dis; P->nfold_inl = (int)id.size();
        P->fadj_built = true;
    }
    *out = AdjointSynthesis{P->d_fadj_Wi, P->d_fadj_pool4i, P->d_fadj_poolLi, P->d_tw, (const FoldDst*)P->d_fold_dst, (const FoldSrc*)P->d_fold_src, P->nfold_dst,
                            FoldSched{(const int4*)P->d_fold_inl_dst, (const int*)P->d_fold_inl_src, P->nfold_inl}};
    return XSQ_OK;
}
}  // namespace xsq

// workspace: that of the inverse transform over the same rows (Z | fr | seg | fft work)
size_t xsq_slicqt_forward_adjoint_workspace(xsq_plan* P, int BC, int64_t n) {
    if (!P || BC <= 0 || n <= 0) return 0;
    return xsq_slicqt_inverse_workspace(P, BC, xsq_plan_num_slices(P, n));
}

int xsq_slicqt_forward_adjoint(xsq_plan* P, const float* gcoef, int BC, int64_t n, float* gx, void* ws, size_t ws_bytes, void* stream_) {
    XSQ_REQUIRE(P && gcoef && gx && ws, "xsq_slicqt_forward_adjoint: null argument");
    XSQ_REQUIRE(BC > 0 && n > 0, "xsq_slicqt_forward_adjoint: BC=%d n=%lld", BC, (long long)n);
    const int S = xsq_plan_num_slices(P, n);
    XSQ_REQUIRE(S >= 2, "xsq_slicqt_forward_adjoint: signal too short");
    const size_t need = xsq_slicqt_forward_adjoint_workspace(P, BC, n);
    XSQ_REQUIRE(need && need <= ws_bytes, "xsq_slicqt_forward_adjoint: workspace too small (%zu needed, %zu given)", need, ws_bytes);
    AdjointSynthesis adj;
    if (int rc = forward_adjoint_tables(P, &adj)) return rc;
    return inverse_impl(P, gcoef, nullptr, 0, BC, S, n, gx, nullptr, ws, ws_bytes, stream_, nullptr, &adj);
}

// ---- the emission of a streaming step: masked inverse of the new slices only, overlap-added onto the carried half ----
size_t xsq_slicqt_inverse_carry_workspace(xsq_plan* P, int BC, int BCx, int S) {
    if (!P || BC <= 0 || BCx <= 0 || S <= 0) return 0;
    const size_t inv = xsq_slicqt_inverse_workspace(P, BC, S);
    if (!inv) return 0;
    return al256((size_t)BCx * S * P->sumFT * 8) + al256((size_t)BC * S * P->sumFT * 4) + inv;
}

int xsq_slicqt_inverse_masked_carry(xsq_plan* P, const float* masks, const float* mix, int BC, int BCx, int S_window, int first, int S,
                                    int shift, int64_t length, float* y, int64_t y_stride, const float* carry_in, float* carry_out,
                                    void* ws, size_t ws_bytes, void* stream_) {
    XSQ_REQUIRE(P && masks && mix && y && carry_out && ws, "xsq_slicqt_inverse_masked_carry: null argument");
    // the mirrored synthesis turns with the parity of the slice's index in the whole stream, which a step does not know
    XSQ_REQUIRE(!P->ntwins, "xsq_slicqt_inverse_masked_carry: a plan with bands across DC (dc_twins, xsq_plan_create_twins) cannot stream");
    XSQ_REQUIRE(BCx > 0 && BC > 0 && BC % BCx == 0, "xsq_slicqt_inverse_masked_carry: %d mix channels do not divide %d mask channels", BCx, BC);
    XSQ_REQUIRE(S >= 1 && first >= 0 && first + S <= S_window, "xsq_slicqt_inverse_masked_carry: slices [%d, %d) of a window of %d", first,
                first + S, S_window);
    XSQ_REQUIRE(shift == 0 || (shift == 1 && carry_in), "xsq_slicqt_inverse_masked_carry: shift=%d (0: the first slice of the stream is among "
                "these; 1: its predecessor's second half is carry_in)", shift);
    const int nblk = S - 1 + shift;              // S slices at positions shift .. S - 1 + shift close the blocks 0 .. nblk - 1
    XSQ_REQUIRE(nblk >= 1 && length >= 1 && length <= (int64_t)nblk * 2 * P->h && y_stride >= length,
                "xsq_slicqt_inverse_masked_carry: %lld samples of %d blocks, row stride %lld", (long long)length, nblk, (long long)y_stride);
    XSQ_REQUIRE(P->nblocks <= TAKE_MAX_BLOCKS && BC + BCx <= 65535, "xsq_slicqt_inverse_masked_carry: %d band blocks, %d channels", P->nblocks, BC);
    const size_t need = xsq_slicqt_inverse_carry_workspace(P, BC, BCx, S);
    XSQ_REQUIRE(need && need <= ws_bytes, "xsq_slicqt_inverse_masked_carry: workspace too small (%zu needed, %zu given)", need, ws_bytes);
    hipStream_t stream = (hipStream_t)stream_;
    char* w = (char*)ws;
    float* Xn = (float*)w; w += al256((size_t)BCx * S * P->sumFT * 8);
    float* Mn = (float*)w; w += al256((size_t)BC * S * P->sumFT * 4);
    TakeArgs a;
    a.Ssrc = S_window; a.Sdst = S; a.s0 = first;
    int64_t per_max = 0;
    for (int j = 0; j < P->nblocks; ++j) {
        a.cum[j] = (int)P->blocks[j].cum; a.T[j] = P->blocks[j].T;
        per_max = std::max<int64_t>(per_max, (int64_t)S * P->blocks[j].F * P->blocks[j].T);
    }
    a.cum[P->nblocks] = (int)P->sumFT;
    a.src[0] = mix; a.dst[0] = Xn; a.C[0] = BCx;
    a.src[1] = masks; a.dst[1] = Mn; a.C[1] = BC;
    { XSQ_PROF("take_slices", stream);
    hipLaunchKernelGGL(k_take_slices, dim3((unsigned)((2 * per_max / 4 + 255) / 256), P->nblocks, BCx + BC), dim3(256), 0, stream, a); }
    XSQ_HIP(hipGetLastError());
    const CarryArgs c{carry_in, carry_out, y_stride, shift, nblk};
    return inverse_impl(P, Xn, Mn, BCx, BC, S, length, y, nullptr, w, ws_bytes - (size_t)(w - (char*)ws), stream_, &c);
}

// ---- remix: R gain-weighted mixes of the four targets through R (not four) inverse transforms ----
static int remix_gains_ok(const float* gains, int R, const char* who) {
    XSQ_REQUIRE(gains, "%s: null gains", who);
    XSQ_REQUIRE(R >= 1 && R <= 4, "%s: R=%d mixes (1..4)", who, R);
    for (int i = 0; i < 4 * R; ++i) XSQ_REQUIRE(std::isfinite(gains[i]), "%s: gain [%d][%d] is not finite", who, i / 4, i % 4);
    return XSQ_OK;
}

size_t xsq_slicqt_remix_workspace(xsq_plan* P, int R, int B, int S, int wiener) {
    if (!P || R < 1 || R > 4 || B <= 0 || S <= 0) return 0;
    const size_t inv = xsq_slicqt_inverse_workspace(P, R * 2 * B, S);
    if (!inv) return 0;
    return al256((size_t)R * 2 * B * S * P->sumFT * (wiener ? 8 : 4)) + inv;
}

int xsq_slicqt_inverse_remix(xsq_plan* P, const float* masks, const float* mix, const float* Y, const float* gains, int R, int B,
                             int S, int64_t length, float* y, const int64_t* row_offsets, void* ws, size_t ws_bytes, void* stream_) {
    if (int rc = remix_gains_ok(gains, R, "xsq_slicqt_inverse_remix")) return rc;
    XSQ_REQUIRE(P && y && ws, "xsq_slicqt_inverse_remix: null argument");
    XSQ_REQUIRE(Y ? (!masks && !mix) : (masks && mix), "xsq_slicqt_inverse_remix: pass masks and mix (mix-phase) or Y (Wiener-EM), not both");
    XSQ_REQUIRE(B > 0 && S >= 2 && 2 * B <= 65535, "xsq_slicqt_inverse_remix: B=%d S=%d", B, S);
    XSQ_REQUIRE(P->nblocks <= REMIX_MAX_BLOCKS, "xsq_slicqt_inverse_remix: %d band blocks (at most %d)", P->nblocks, REMIX_MAX_BLOCKS);
    const int wiener = Y ? 1 : 0, BC = R * 2 * B;
    const size_t need = xsq_slicqt_remix_workspace(P, R, B, S, wiener);
    XSQ_REQUIRE(need && need <= ws_bytes, "xsq_slicqt_inverse_remix: workspace too small (%zu needed, %zu given)", need, ws_bytes);
    const size_t comb_bytes = al256((size_t)BC * S * P->sumFT * (wiener ? 8 : 4));
    float* comb = (float*)ws;
    RemixArgs a;
    a.src = Y ? Y : masks; a.dst = comb; a.nch = 2 * B; a.R = R; a.S = S; a.cplx = wiener ? 2 : 1;
    for (int t = 0; t < 4; ++t) a.use[t] = 0;
    for (int r = 0; r < 4; ++r)
        for (int t = 0; t < 4; ++t) {
            a.g[r][t] = r < R ? gains[4 * r + t] : 0.f;
            if (r < R && gains[4 * r + t] != 0.f) a.use[t] = 1;
        }
    int64_t per_max = 0;
    for (int j = 0; j < P->nblocks; ++j) {
        a.cum[j] = (int)P->blocks[j].cum;
        per_max = std::max<int64_t>(per_max, (int64_t)S * P->blocks[j].F * P->blocks[j].T * a.cplx);
    }
    a.cum[P->nblocks] = (int)P->sumFT;
    hipStream_t stream = (hipStream_t)stream_;
    { XSQ_PROF("remix_combine", stream);
    hipLaunchKernelGGL(k_remix_combine, dim3((unsigned)((per_max / 4 + 255) / 256), P->nblocks, 2 * B), dim3(256), 0, stream, a); }
    XSQ_HIP(hipGetLastError());
    char* inv_ws = (char*)ws + comb_bytes;
    if (wiener) return inverse_impl(P, comb, nullptr, 0, BC, S, length, y, row_offsets, inv_ws, ws_bytes - comb_bytes, stream_);
    return inverse_impl(P, mix, comb, 2 * B, BC, S, length, y, row_offsets, inv_ws, ws_bytes - comb_bytes, stream_);
}

}  // extern "C"
