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
// estimates: 8B) and the real arena of the masks (8B) share it: an element is a float2 in the former, a float in the latter.
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

// The workgroup's NV accumulators (16 sums; NV = 17: and a maximum in slot 16) over WAVES wavefronts: wavefront butterfly, then
// the tree over the wave partials.  No atomics: bitwise reproducible.  Thread i < NV stores the total of slot i to out[i] (LDS or
// global memory).  `red` may be written again after the workgroup's next barrier.
template <int WAVES, int NV>
__device__ inline void reduce(const float (&acc)[NV], float (*red)[NV], float* out) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        float v = acc[i];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float o = __shfl_xor(v, off, 64);
            v = (i == 16) ? fmaxf(v, o) : v + o;
        }
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][i] = v;
    }
    __syncthreads();
    if (threadIdx.x < NV) {
        const int i = threadIdx.x;
        if (NV == 17 && i == 16) out[i] = tree<WAVES, true>(red, i);
        else out[i] = tree<WAVES, false>(red, i);
    }
}

// ---- R and the point solve ---------------------------------------------------------------------------------------------
struct WR {                     // R_j = [[r00, r01], [conj(r01), r11]] of the four sources
    float r00[4], r11[4];
    float2 r01[4];
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

// the same on a statistics slot in place: st[0..15] sums -> R, st[20..23] = den
__device__ inline void sums_to_R_slot(float* st, int j, const float* sums, float inv_ma2) {
    float r00, r11, den;
    float2 r01;
    sums_to_R(sums[4 * j], sums[4 * j + 1], sums[4 * j + 2], sums[4 * j + 3], inv_ma2, r00, r11, r01, den);
    st[4 * j] = r00;
    st[4 * j + 1] = r11;
    st[4 * j + 2] = r01.x;
    st[4 * j + 3] = r01.y;
    st[20 + j] = den;
}

__device__ inline void load_R(const float* __restrict__ st, WR& R) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
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
__device__ inline WInv invert_cxx(const WR& R, const float (&v)[4]) {
    const float reg = sqrtf(FLT_EPSILON);
    float c00 = reg, c11 = reg;
    float2 c01 = make_float2(0.f, 0.f);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
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
__device__ inline void mul_R(const WR& R, int j, float2 z0, float2 z1, float2& o0, float2& o1) {
    const float2 a = cmul(R.r01[j], z1);
    const float2 b = cmulc(z0, R.r01[j]);      // conj(R01) * z0
    o0 = make_float2(R.r00[j] * z0.x + a.x, R.r00[j] * z0.y + a.y);
    o1 = make_float2(b.x + R.r11[j] * z1.x, b.y + R.r11[j] * z1.y);
}

// y_j = v_j R_j z
__device__ inline void source(const WR& R, int j, float vj, float2 z0, float2 z1, float2& y0, float2& y1) {
    float2 o0, o1;
    mul_R(R, j, z0, z1, o0, o1);
    y0 = make_float2(vj * o0.x, vj * o0.y);
    y1 = make_float2(vj * o1.x, vj * o1.y);
}

// one time-frequency point of the filter: estimates y (unscaled), statistics slot st -> filtered estimates o
__device__ inline void wiener_point(const float* __restrict__ st, float2 x0, float2 x1, const float2 (&y)[4][2], float2 (&o)[4][2]) {
    const float inv_ma2 = st[16];
    WR R;
    load_R(st, R);
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = power(y[j][0], y[j][1], inv_ma2);
    float2 z0, z1;
    solve(invert_cxx(R, v), x0, x1, z0, z1);
#pragma unroll
    for (int j = 0; j < 4; ++j) source(R, j, v[j], z0, z1, o[j][0], o[j][1]);
}

}  // namespace xsq
