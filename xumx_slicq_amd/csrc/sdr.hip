// The SDR term of the reference's training loss on waveforms, gfx950.
//
// Reference: xumx_slicq_v2/loss.py:5-34 (SDRLossCriterion: auraloss.time.SDSDRLoss() of the 4 + 6 + 4 one-, two- and
// three-target sums of estimated vs target waveforms, / 14).  SDSDRLoss defaults (zero_mean, eps = 1e-8, mean over the
// (B, 2) rows), for a row with estimate p and target t of n samples, both centred:
//   alpha = <p, t> / (<t, t> + eps)
//   loss  = -10 log10( |alpha t|^2 / (|p - t|^2 + eps) + eps )                  (the residual is p - t, NOT p - alpha t)
// Every sum the 14 combinations of a row need is linear or bilinear in the four estimates and four targets of the row, so the
// combinations are never formed.  With e_i = p_i - t_i, 44 moments per row suffice: sum e_i, sum t_i (8), sum e_i t_j (16),
// sum t_i t_j and sum e_i e_j for i <= j (10 + 10).  The gradient of one combination's row loss with respect to its estimate
// is  A t_c[k] + B e_c[k]  (t_c, e_c centred: its mean over k is zero, the centring needs no second correction), so
//   gy[i, row, k] = sum_j ( a_ij t_j[k] + b_ij e_j[k] ) + gamma_i            -- a 4 x 9 coefficient matrix per row.
// Pass 1 (k_sdr_moments) reads 8 floats per sample and reduces the moments: products and sums in fp64, fixed order, no
// atomics (bitwise reproducible); k_sdr_finalise turns them into the 14 row losses and the matrix, in double; pass 2
// (k_sdr_grad) reads the same 8 floats and writes the 4 gradients.  A silent target gives alpha = 0, row loss 80, gradient 0.
#include "../../include/xumx_slicq_hip.h"
#include "common.h"
#include "prof.h"

namespace xsq {

constexpr int SDR_NM = 44;            // moments per row
constexpr int SDR_CHUNK = 4096;       // samples of one workgroup of pass 1
constexpr int SDR_M_SE = 0, SDR_M_ST = 4, SDR_M_ET = 8, SDR_M_TT = 24, SDR_M_EE = 34;
constexpr double SDR_EPS = 1e-8;

// index of the pair (i <= j) among the 10 of a symmetric 4 x 4: 00 01 02 03 11 12 13 22 23 33
__host__ __device__ constexpr int sdr_sym(int i, int j) { return i * 4 - i * (i - 1) / 2 + (j - i); }

// waveforms (4, R, n): source i of row r at base + (i * R + r) * n.  grid (chunks, R).
__global__ __launch_bounds__(256) void k_sdr_moments(const float* __restrict__ pred, const float* __restrict__ tgt,
                                                      double* __restrict__ partial, int R, int64_t n) {
    const int r = blockIdx.y;
    const int64_t k0 = (int64_t)blockIdx.x * SDR_CHUNK, k1 = k0 + SDR_CHUNK < n ? k0 + SDR_CHUNK : n;
    double acc[SDR_NM];
#pragma unroll
    for (int m = 0; m < SDR_NM; ++m) acc[m] = 0.0;
    for (int64_t k = k0 + threadIdx.x; k < k1; k += 256) {
        double e[4], t[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float pv = pred[((int64_t)i * R + r) * n + k], tv = tgt[((int64_t)i * R + r) * n + k];
            e[i] = (double)(pv - tv);
            t[i] = (double)tv;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            acc[SDR_M_SE + i] += e[i];
            acc[SDR_M_ST + i] += t[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[SDR_M_ET + 4 * i + j] += e[i] * t[j];
#pragma unroll
            for (int j = i; j < 4; ++j) {
                acc[SDR_M_TT + sdr_sym(i, j)] += t[i] * t[j];
                acc[SDR_M_EE + sdr_sym(i, j)] += e[i] * e[j];
            }
        }
    }
    __shared__ double red[4][SDR_NM];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int m = 0; m < SDR_NM; ++m) {
        const double v = wave_sum(acc[m]);
        if (lane == 0) red[wave][m] = v;
    }
    __syncthreads();
    if (threadIdx.x < SDR_NM)
        partial[((int64_t)r * gridDim.x + blockIdx.x) * SDR_NM + threadIdx.x] =
            ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// the members of the 14 combinations as bit sets, in the reference's order (loss.py:17-32)
__constant__ int SDR_COMBO[14] = {1, 2, 4, 8, 3, 5, 9, 6, 10, 12, 7, 11, 13, 14};

// One workgroup of 64 threads per row: moments (fixed-order sum over the chunks) -> 14 row losses and the 4 x 9 matrix of
// pass 2, scaled by `weight` = scale / (14 R): gy is then the gradient of scale * criterion.  rowloss: [R][14] row losses, then the
// two scalars of every combination's gradient  A t_c + B e_c  (weight included) as [R][14] each.
__global__ __launch_bounds__(64) void k_sdr_finalise(const double* __restrict__ partial, int nchunks, int64_t n, double weight,
                                                      double* __restrict__ rowloss, float* __restrict__ coef) {
    const int R = gridDim.x;
    const int r = blockIdx.x, tid = threadIdx.x;
    __shared__ double mom[SDR_NM];
    __shared__ double cA[14], cB[14], cG[14];
    if (tid < SDR_NM) {
        double a = 0.0;
        for (int c = 0; c < nchunks; ++c) a += partial[((int64_t)r * nchunks + c) * SDR_NM + tid];
        mom[tid] = a;
    }
    __syncthreads();
    if (tid < 14) {
        const int set = SDR_COMBO[tid];
        double Se = 0.0, St = 0.0, ET = 0.0, TT = 0.0, EE = 0.0;
        for (int i = 0; i < 4; ++i) {
            if (!(set >> i & 1)) continue;
            Se += mom[SDR_M_SE + i];
            St += mom[SDR_M_ST + i];
            for (int j = 0; j < 4; ++j) {
                if (!(set >> j & 1)) continue;
                ET += mom[SDR_M_ET + 4 * i + j];
                TT += mom[SDR_M_TT + (i <= j ? sdr_sym(i, j) : sdr_sym(j, i))];
                EE += mom[SDR_M_EE + (i <= j ? sdr_sym(i, j) : sdr_sym(j, i))];
            }
        }
        const double inv_n = 1.0 / (double)n;
        const double cet = ET - Se * St * inv_n;
        const double ctt = fmax(TT - St * St * inv_n, 0.0), cee = fmax(EE - Se * Se * inv_n, 0.0);      // (sums of squares of centred signals)
        const double alpha = (cet + ctt) / (ctt + SDR_EPS);
        const double den = cee + SDR_EPS;
        const double ratio = alpha * alpha * ctt / den + SDR_EPS;
        rowloss[r * 14 + tid] = -10.0 * log10(ratio);
        const double K = -10.0 / (2.302585092994045684 * ratio) * weight;
        const double A = K * 2.0 * alpha * ctt / (den * (ctt + SDR_EPS));
        const double Bc = -K * 2.0 * alpha * alpha * ctt / (den * den);
        cA[tid] = A; cB[tid] = Bc; cG[tid] = -(A * St + Bc * Se) * inv_n;
        rowloss[(R + r) * 14 + tid] = A;
        rowloss[(2 * R + r) * 14 + tid] = Bc;
    }
    __syncthreads();
    if (tid < 36) {          // entry (i, col): col 0..3 on t_j, 4..7 on e_j, 8 the constant
        const int i = tid / 9, col = tid - 9 * i, j = col & 3;
        double v = 0.0;
        for (int c = 0; c < 14; ++c) {
            const int set = SDR_COMBO[c];
            if (!(set >> i & 1)) continue;
            if (col == 8) v += cG[c];
            else if (set >> j & 1) v += col < 4 ? cA[c] : cB[c];
        }
        coef[r * 36 + tid] = (float)v;
    }
}

// the criterion: mean over rows and combinations; one wave, fixed order (lane-strided sums, then the shuffle tree)
__global__ __launch_bounds__(64) void k_sdr_total(const double* __restrict__ rowloss, int R, double* __restrict__ out) {
    double a = 0.0;
    for (int i = threadIdx.x; i < 14 * R; i += 64) a += rowloss[i];
    a = wave_sum(a);
    if (threadIdx.x == 0) out[0] = a / (14.0 * (double)R);
}

// grid (ceil(n / 1024), R): four samples per thread, 256 apart
__global__ __launch_bounds__(256) void k_sdr_grad(const float* __restrict__ pred, const float* __restrict__ tgt,
                                                   const float* __restrict__ coef, float* __restrict__ gy, int R, int64_t n) {
    const int r = blockIdx.y;
    float cf[36];
#pragma unroll
    for (int m = 0; m < 36; ++m) cf[m] = coef[r * 36 + m];
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int64_t k = (int64_t)blockIdx.x * 1024 + it * 256 + threadIdx.x;
        if (k >= n) break;
        float e[4], t[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float pv = pred[((int64_t)i * R + r) * n + k];
            t[i] = tgt[((int64_t)i * R + r) * n + k];
            e[i] = pv - t[i];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float v = cf[9 * i + 8];
#pragma unroll
            for (int j = 0; j < 4; ++j) v = fmaf(cf[9 * i + j], t[j], fmaf(cf[9 * i + 4 + j], e[j], v));
            gy[((int64_t)i * R + r) * n + k] = v;
        }
    }
}

static inline int64_t sdr_chunks(int64_t n) { return (n + SDR_CHUNK - 1) / SDR_CHUNK; }

// pred / target (4, R, n) -> out: DEVICE double[1 + 42 R] = criterion, then the row losses [row][combination] it is the mean of, then
// the gradient scalars A and B of every (row, combination) (k_sdr_finalise);
// gy (4, R, n) or null = scale * d criterion / d pred
int sdr_loss(const float* pred, const float* target, int R, int64_t n, float scale, double* out, float* gy, void* ws, hipStream_t stream) {
    const int64_t nch = sdr_chunks(n);
    char* w = (char*)ws;
    double* partial = (double*)w; w += al256((size_t)R * nch * SDR_NM * 8);
    double* rowloss = out + 1;
    float* coef = (float*)w;
    { XSQ_PROF("sdr_moments", stream);
      hipLaunchKernelGGL(k_sdr_moments, dim3((unsigned)nch, R), dim3(256), 0, stream, pred, target, partial, R, n); }
    { XSQ_PROF("sdr_finalise", stream);
      hipLaunchKernelGGL(k_sdr_finalise, dim3(R), dim3(64), 0, stream, partial, (int)nch, n, (double)scale / (14.0 * R), rowloss, coef);
      hipLaunchKernelGGL(k_sdr_total, dim3(1), dim3(64), 0, stream, rowloss, R, out); }
    if (gy) { XSQ_PROF("sdr_grad", stream);
      hipLaunchKernelGGL(k_sdr_grad, dim3((unsigned)((n + 1023) / 1024), R), dim3(256), 0, stream, pred, target, coef, gy, R, n); }
    XSQ_HIP(hipGetLastError());
    return XSQ_OK;
}

}  // namespace xsq

using namespace xsq;

extern "C" {

size_t xsq_sdr_loss_workspace(int B, int64_t n) {
    if (B <= 0 || n <= 0 || 2 * (int64_t)B > 65535 || sdr_chunks(n) > 0x7fffffff) return 0;
    const size_t R = 2 * (size_t)B;
    return al256(R * sdr_chunks(n) * SDR_NM * 8) + al256(R * 36 * 4) + 256;
}

static int sdr_args_ok(const char* who, const float* pred, const float* target, int B, int64_t n, double* out, void* ws, size_t ws_bytes) {
    XSQ_REQUIRE(pred && target && out && ws, "%s: null argument", who);
    XSQ_REQUIRE(B > 0 && n > 0, "%s: B=%d n=%lld", who, B, (long long)n);
    const size_t need = xsq_sdr_loss_workspace(B, n);
    XSQ_REQUIRE(need && ws_bytes >= need, "%s: workspace too small (%zu needed, %zu given)", who, need, ws_bytes);
    return XSQ_OK;
}

int xsq_sdr_loss_forward(const float* pred, const float* target, int B, int64_t n, double* out, void* ws, size_t ws_bytes, void* stream_) {
    if (int rc = sdr_args_ok("xsq_sdr_loss_forward", pred, target, B, n, out, ws, ws_bytes)) return rc;
    return sdr_loss(pred, target, 2 * B, n, 1.f, out, nullptr, ws, (hipStream_t)stream_);
}

int xsq_sdr_loss_backward(const float* pred, const float* target, int B, int64_t n, float scale, double* out, float* gy, void* ws,
                          size_t ws_bytes, void* stream_) {
    if (int rc = sdr_args_ok("xsq_sdr_loss_backward", pred, target, B, n, out, ws, ws_bytes)) return rc;
    XSQ_REQUIRE(gy, "xsq_sdr_loss_backward: null argument");
    return sdr_loss(pred, target, 2 * B, n, scale, out, gy, ws, (hipStream_t)stream_);
}

}  // extern "C"
