// Device arithmetic of the Wiener-EM iteration (norbert/__init__.py:10-150), written once: the kernels of wiener.hip that
// read and write the arena and the window-resident kernel of wiener_iter.h all go through these functions, so "the two-step
// form, the masked form, the looped form and the resident form give the same bits" holds because they run the same code.
// Notation: wiener.hip.
#pragma once
#include <cfloat>
#include <cstdint>

#include <hip/hip_runtime.h>

namespace xsq {

static const int STAT = 24;   // floats per (row, window): 4 sources x (C00, C11, Re C01, Im C01), max|x|^2, pad[3],
                              // 4 x 1/(sum_n v + eps) (kept for the backward pass)

// The slot of J sources.  J = 4 is the layout above (the training backward reads it); J = 5 (the four targets and the residual
// of norbert.contrib.residual_model) has 20 sums, max|x|^2 at [20], pad[3], 5 denominators at [24], pad[3].
template <int J> struct Slot;
template <> struct Slot<4> { static constexpr int N = STAT, MAX = 16, DEN = 20; };
template <> struct Slot<5> { static constexpr int N = 32, MAX = 20, DEN = 24; };

// How the initial estimates of a time-frequency point come about (norbert.wiener :247-251): the mixture phase on the magnitudes
// v_j (use_softmask=False) or the ratio mask x v_j / (eps + sum_j v_j) (softmask, :263-309).  Kernels fed by estimates take them
// as given.
enum class Start { MixPhase, Softmask };

struct WRow {          // one (block, batch item, bin) row of the arena
    int F, T;          // block geometry
    int b, f;          // batch item, bin
    int nrows;         // rows sharing this row's window maximum (batch_group * F)
    int64_t cum;       // sum over earlier blocks of F*T
    int64_t stat;      // float offset of this row's window 0 in the stats buffer
};

__device__ inline float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ inline float2 cmulc(float2 a, float2 b) { return make_float2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y); }  // a * conj(b)
__device__ inline float abs2(float2 a) { return a.x * a.x + a.y * a.y; }

// arena index of (chan, f, frame n) for a block; nchan = packed channels of the arena.  The complex arenas (mix: 2B channels,
// estimates: 2JB) and the real arena of the masks (8B) share it: an element is a float2 in the former, a float in the latter.
__device__ inline int64_t aidx(const WRow& r, int nchan, int S, int chan, int64_t n) {
    return (int64_t)nchan * S * r.cum + ((int64_t)chan * r.F + r.f) * ((int64_t)S * r.T) + n;
}

// frames [n0, n1) of window w of a row
struct WWin {
    int64_t N, n0, n1;
};
__device__ inline WWin window_of(const WRow& r, int S, int w, int win_len) {
    WWin W;
    W.N = (int64_t)S * r.T;
    W.n0 = (int64_t)w * win_len;
    W.n1 = W.n0 + win_len < W.N ? W.n0 + win_len : W.N;
    return W;
}

// ---- statistics --------------------------------------------------------------------------------------------------------
// one frame of source j into the four sums C00, C11, Re C01, Im C01 of y y^H
template <int NV>
__device__ inline void accumulate(float (&acc)[NV], int j, float2 y0, float2 y1) {
    const float2 c01 = cmulc(y0, y1);
    acc[4 * j + 0] += abs2(y0);
    acc[4 * j + 1] += abs2(y1);
    acc[4 * j + 2] += c01.x;
    acc[4 * j + 3] += c01.y;
}

// slot i of the WAVES wave partials in LDS: fixed-order pairwise tree, ((p0 . p1) . (p2 . p3)) . ...
template <int WAVES, bool MAX, int NV>
__device__ inline float tree(const float (*red)[NV], int i) {
    float p[WAVES];
#pragma unroll
    for (int k = 0; k < WAVES; ++k) p[k] = red[k][i];
#pragma unroll
    for (int s = 1; s < WAVES; s <<= 1)
#pragma unroll
        for (int k = 0; k < WAVES; k += 2 * s) p[k] = MAX ? fmaxf(p[k], p[k + s]) : p[k] + p[k + s];
    return p[0];
}

// The workgroup's NV accumulators (4J sums; NV = 4J + 1: and a maximum in the last slot) over WAVES wavefronts: wavefront butterfly, then
// the tree over the wave partials.  No atomics: bitwise reproducible.  Thread i < NV stores the total of slot i to out[i] (LDS or
// global memory).  `red` may be written again after the workgroup's next barrier.
template <int WAVES, int NV>
__device__ inline void reduce(const float (&acc)[NV], float (*red)[NV], float* out) {
    constexpr bool HASMAX = NV % 4 == 1;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        float v = acc[i];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float o = __shfl_xor(v, off, 64);
            v = (HASMAX && i == NV - 1) ? fmaxf(v, o) : v + o;
        }
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][i] = v;
    }
    __syncthreads();
    if (threadIdx.x < NV) {
        const int i = threadIdx.x;
        if (HASMAX && i == NV - 1) out[i] = tree<WAVES, true>(red, i);
        else out[i] = tree<WAVES, false>(red, i);
    }
}

// ---- R and the point solve ---------------------------------------------------------------------------------------------
template <int J>
struct WR {                     // R_j = [[r00, r01], [conj(r01), r11]] of the J sources
    float r00[J], r11[J];
    float2 r01[J];
};

// raw sums of one source -> R and den = 1 / (sum_n v' + eps)   (norbert :491-493).  inv_ma2 = 1 / ma^2 brings sums of
// unscaled estimates to scaled units; sums taken in scaled units pass a literal 1.
__device__ inline void sums_to_R(float s00, float s11, float s01x, float s01y, float inv_ma2, float& r00, float& r11, float2& r01,
                                 float& den) {
    const float c00 = s00 * inv_ma2, c11 = s11 * inv_ma2;
    den = 1.f / (0.5f * (c00 + c11) + FLT_EPSILON);         // sum_n mean_c |y'|^2 + eps
    r00 = c00 * den;
    r11 = c11 * den;
    r01 = make_float2(s01x * inv_ma2 * den, s01y * inv_ma2 * den);
}

// the same on a statistics slot in place: st[0..4J-1] sums -> R, st[DEN..DEN+J-1] = den
template <int J>
__device__ inline void sums_to_R_slot(float* st, int j, const float* sums, float inv_ma2) {
    float r00, r11, den;
    float2 r01;
    sums_to_R(sums[4 * j], sums[4 * j + 1], sums[4 * j + 2], sums[4 * j + 3], inv_ma2, r00, r11, r01, den);
    st[4 * j] = r00;
    st[4 * j + 1] = r11;
    st[4 * j + 2] = r01.x;
    st[4 * j + 3] = r01.y;
    st[Slot<J>::DEN + j] = den;
}

template <int J>
__device__ inline void load_R(const float* __restrict__ st, WR<J>& R) {
#pragma unroll
    for (int j = 0; j < J; ++j) {
        R.r00[j] = st[4 * j];
        R.r11[j] = st[4 * j + 1];
        R.r01[j] = make_float2(st[4 * j + 2], st[4 * j + 3]);
    }
}

// v' = mean_c |y'|^2 of an estimate in unscaled units (inv_ma2 = 1 / ma^2) or in scaled ones (a literal 1)
__device__ inline float power(float2 y0, float2 y1, float inv_ma2) { return 0.5f * (abs2(y0) * inv_ma2 + abs2(y1) * inv_ma2); }

// Cxx^-1 = [[i00, i01], [i10, i11]] with Cxx = sum_j v_j R_j + sqrt(eps) I; analytic inverse (norbert _invert :337-346)
struct WInv {
    float i00, i11;
    float2 i01, i10;
};
template <int J>
__device__ inline WInv invert_cxx(const WR<J>& R, const float (&v)[J]) {
    const float reg = sqrtf(FLT_EPSILON);
    float c00 = reg, c11 = reg;
    float2 c01 = make_float2(0.f, 0.f);
#pragma unroll
    for (int j = 0; j < J; ++j) {
        c00 += v[j] * R.r00[j];
        c11 += v[j] * R.r11[j];
        c01.x += v[j] * R.r01[j].x;
        c01.y += v[j] * R.r01[j].y;
    }
    const float det = c00 * c11 - abs2(c01);
    const float idet = 1.f / det;
    WInv I;
    I.i00 = c11 * idet;
    I.i11 = c00 * idet;
    I.i01 = make_float2(-c01.x * idet, -c01.y * idet);    // -c01/det
    I.i10 = make_float2(-c01.x * idet, c01.y * idet);     // -conj(c01)/det
    return I;
}

// z = Cxx^-1 a
__device__ inline void solve(const WInv& I, float2 a0, float2 a1, float2& z0, float2& z1) {
    z0 = make_float2(I.i00 * a0.x + (I.i01.x * a1.x - I.i01.y * a1.y), I.i00 * a0.y + (I.i01.x * a1.y + I.i01.y * a1.x));
    z1 = make_float2((I.i10.x * a0.x - I.i10.y * a0.y) + I.i11 * a1.x, (I.i10.x * a0.y + I.i10.y * a0.x) + I.i11 * a1.y);
}

// R_j z
template <int J>
__device__ inline void mul_R(const WR<J>& R, int j, float2 z0, float2 z1, float2& o0, float2& o1) {
    const float2 a = cmul(R.r01[j], z1);
    const float2 b = cmulc(z0, R.r01[j]);      // conj(R01) * z0
    o0 = make_float2(R.r00[j] * z0.x + a.x, R.r00[j] * z0.y + a.y);
    o1 = make_float2(b.x + R.r11[j] * z1.x, b.y + R.r11[j] * z1.y);
}

// y_j = v_j R_j z
template <int J>
__device__ inline void source(const WR<J>& R, int j, float vj, float2 z0, float2 z1, float2& y0, float2& y1) {
    float2 o0, o1;
    mul_R(R, j, z0, z1, o0, o1);
    y0 = make_float2(vj * o0.x, vj * o0.y);
    y1 = make_float2(vj * o1.x, vj * o1.y);
}

// one time-frequency point of the filter: estimates y (unscaled), statistics slot st -> filtered estimates o
template <int J>
__device__ inline void wiener_point(const float* __restrict__ st, float2 x0, float2 x1, const float2 (&y)[J][2], float2 (&o)[J][2]) {
    const float inv_ma2 = st[Slot<J>::MAX];
    WR<J> R;
    load_R(st, R);
    float v[J];
#pragma unroll
    for (int j = 0; j < J; ++j) v[j] = power(y[j][0], y[j][1], inv_ma2);
    float2 z0, z1;
    solve(invert_cxx(R, v), x0, x1, z0, z1);
#pragma unroll
    for (int j = 0; j < J; ++j) source(R, j, v[j], z0, z1, o[j][0], o[j][1]);
}

// ---- the initial estimates of one channel of one point -------------------------------------------------------------------
// x/|x| for every finite x.  re^2 + im^2 is a normal fp32 number for |x| in about (1.1e-19, 1.8e19): there the plain form
// is used (and its bits kept).  Below, the sum of squares is subnormal or 0 (the phase would be lost: x = (1e-30, 1e-30) gave
// (1, 0)), above it is inf (the output was 0): x is first divided by max(|re|, |im|), which puts the modulus in [1, sqrt 2].
__device__ __forceinline__ float2 unit_phase(float2 x) {
    const float a2 = x.x * x.x + x.y * x.y;
    if (a2 >= FLT_MIN && a2 <= FLT_MAX) {
        const float ax = sqrtf(a2);
        return make_float2(x.x / ax, x.y / ax);
    }
    const float s = fmaxf(fabsf(x.x), fabsf(x.y));
    if (!(s > 0.f)) return make_float2(1.f, 0.f);            // angle(0) = 0
    const float re = x.x / s, im = x.y / s;
    const float ax = sqrtf(re * re + im * im);
    return make_float2(re / ax, im / ax);
}

// The J starts y of one channel from the mix x and a[0..3]: the sigmoid masks m_j (MASKS; v_j = m_j |x|, one fp32 rounding, the
// products the fp32 oracle forms) or the magnitudes v_j themselves.
//   J = 5      v_4 = relu(max(|x|, eps) - (((v_0 + v_1) + v_2) + v_3))   (norbert/contrib.py:11-77 with alpha = 1; F.threshold
//              replaces values <= eps).  Never stored as a magnitude: formed here, as the frame is loaded.
//   MixPhase   y_j = m_j x for the targets of the masked forms (what every masked kernel formed before there were options),
//              v_j x/|x| otherwise; the residual is v_4 x/|x|, real where x = 0 (angle(0) = 0).
//   Softmask   y_j = x v_j / (eps + sum_j v_j), the sum over all J sources.
template <int J, Start ST, bool MASKS>
__device__ inline void start_channel(float2 x, const float (&a)[4], float2 (&y)[J]) {
    if constexpr (J == 4 && ST == Start::MixPhase && MASKS) {
#pragma unroll
        for (int j = 0; j < 4; ++j) y[j] = make_float2(a[j] * x.x, a[j] * x.y);
    } else {
        const float ax = sqrtf(abs2(x));
        float v[J];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = MASKS ? a[j] * ax : a[j];
        const float tot4 = ((v[0] + v[1]) + v[2]) + v[3];
        if constexpr (J == 5) v[4] = fmaxf((ax > FLT_EPSILON ? ax : FLT_EPSILON) - tot4, 0.f);
        if constexpr (ST == Start::Softmask) {
            const float den = FLT_EPSILON + (J == 5 ? tot4 + v[J - 1] : tot4);
#pragma unroll
            for (int j = 0; j < J; ++j) {
                const float g = v[j] / den;
                y[j] = make_float2(g * x.x, g * x.y);
            }
        } else {
            const float2 u = unit_phase(x);
#pragma unroll
            for (int j = 0; j < J; ++j) {
                if (MASKS && j < 4) y[j] = make_float2(a[j] * x.x, a[j] * x.y);
                else y[j] = make_float2(v[j] * u.x, v[j] * u.y);
            }
        }
    }
}

// ---- the ideal-mask oracle: one channel of one point from the coefficients of the four true sources ------------------------
// (xumx_slicq_v2/slicqfinder.py:43-117.)  The mix is their sum, formed as the reference forms it on the real and on the
// imaginary part: model = eps, then model += s_j + eps per source (slicqfinder.py:57,71; eps = 1e-10, five of them in all).
// The magnitudes are v_j = |s_j| and the starts v_j m/|m| are those of start_channel from magnitudes (angle(0) = 0).
static constexpr float ORACLE_EPS = 1.0e-10f;

__device__ inline void sources_channel(const float2 (&s)[4], float2& m, float2 (&y)[4]) {
    m = make_float2(ORACLE_EPS, ORACLE_EPS);
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        m.x += s[j].x + ORACLE_EPS;
        m.y += s[j].y + ORACLE_EPS;
        v[j] = sqrtf(abs2(s[j]));
    }
    start_channel<4, Start::MixPhase, false>(m, v, y);
}

}  // namespace xsq
