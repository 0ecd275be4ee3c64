// More than one EM iteration of the Wiener filter (norbert/__init__.py:133-148, the loop `for it in range(iterations)`
// of expectation_maximization; :247-260, wiener: ONE scaling by max(1, 0.1 max|x|) around all iterations).  Included by
// wiener.hip inside namespace xsq, after WRow / cidx / ridx / cmul / cmulc / STAT.
//
// Two forms.
//   looped    iteration 1 is the three launches of wiener.hip; every further iteration is k_wiener_stats_iter (raw sums of
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

static constexpr int RES_THREADS = 1024;
static constexpr int RES_FPT = 5;                                   // frames per thread
static constexpr int RES_WAVES = RES_THREADS / 64;
static constexpr int RES_MAX_WINDOW = RES_THREADS * RES_FPT;        // 5120 >= the default window of 5000 frames

// ---- looped form: statistics of the current estimates + R, one workgroup per (row, window) ---------------------------
// st[16] holds 1/ma^2 (k_wiener_finalize of iteration 1) and is left alone; st[0..15] and st[20..23] are rewritten.
__global__ __launch_bounds__(256) void k_wiener_stats_iter(const float2* __restrict__ Y, const WRow* __restrict__ rows,
                                                            const int* __restrict__ work, float* __restrict__ stats, int Bn,
                                                            int S, int win_len) {
    const int row = work[2 * blockIdx.x], w = work[2 * blockIdx.x + 1];
    const WRow r = rows[row];
    const int64_t N = (int64_t)S * r.T;
    const int64_t n0 = (int64_t)w * win_len;
    const int64_t n1 = n0 + win_len < N ? n0 + win_len : N;
    float acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    const float2* y00 = Y + cidx(r, 8 * Bn, S, r.b * 2, 0);              // target 0, channel 0 of this row
    const int64_t cstride = (int64_t)r.F * N, jstride = (int64_t)Bn * 2 * cstride;
    for (int64_t n = n0 + threadIdx.x; n < n1; n += 256) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float2 y0 = y00[j * jstride + n], y1 = y00[j * jstride + cstride + n];
            const float2 c01 = cmulc(y0, y1);
            acc[4 * j + 0] += y0.x * y0.x + y0.y * y0.y;
            acc[4 * j + 1] += y1.x * y1.x + y1.y * y1.y;
            acc[4 * j + 2] += c01.x;
            acc[4 * j + 3] += c01.y;
        }
    }
    __shared__ float red[4][16];
    __shared__ float tot[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        float v = acc[i];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][i] = v;
    }
    __syncthreads();
    if (threadIdx.x < 16) tot[threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
    __syncthreads();
    if (threadIdx.x < 4) {                                               // the arithmetic of k_wiener_finalize, per source
        const int j = threadIdx.x;
        float* st = stats + r.stat + (int64_t)w * STAT;
        const float inv_ma2 = st[16];
        const float c00 = tot[4 * j] * inv_ma2, c11 = tot[4 * j + 1] * inv_ma2;
        const float den = 1.f / (0.5f * (c00 + c11) + FLT_EPSILON);
        st[4 * j] = c00 * den;
        st[4 * j + 1] = c11 * den;
        st[4 * j + 2] = tot[4 * j + 2] * inv_ma2 * den;
        st[4 * j + 3] = tot[4 * j + 3] * inv_ma2 * den;
        st[20 + j] = den;
    }
}

// ---- window-resident form ---------------------------------------------------------------------------------------------
struct ResR {                   // R_j = [[r00, r01], [conj(r01), r11]] of the four sources
    float r00[4], r11[4];
    float2 r01[4];
};

// sums (C00, C11, Re C01, Im C01 per source, already in scaled units) -> R   (norbert :491-493)
__device__ inline void res_R(const float (&s)[16], ResR& R) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float den = 1.f / (0.5f * (s[4 * j] + s[4 * j + 1]) + FLT_EPSILON);
        R.r00[j] = s[4 * j] * den;
        R.r11[j] = s[4 * j + 1] * den;
        R.r01[j] = make_float2(s[4 * j + 2] * den, s[4 * j + 3] * den);
    }
}

// z = Cxx^-1 x with Cxx = sum_j v_j R_j + sqrt(eps) I   (the expression tree of wiener_point)
__device__ inline void res_solve(const ResR& R, const float (&v)[4], float2 x0, float2 x1, float2& z0, float2& z1) {
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
    const float det = c00 * c11 - (c01.x * c01.x + c01.y * c01.y);
    const float idet = 1.f / det;
    const float i00 = c11 * idet, i11 = c00 * idet;
    const float2 i01 = make_float2(-c01.x * idet, -c01.y * idet);
    const float2 i10 = make_float2(-c01.x * idet, c01.y * idet);
    z0 = make_float2(i00 * x0.x + (i01.x * x1.x - i01.y * x1.y), i00 * x0.y + (i01.x * x1.y + i01.y * x1.x));
    z1 = make_float2((i10.x * x0.x - i10.y * x0.y) + i11 * x1.x, (i10.x * x0.y + i10.y * x0.x) + i11 * x1.y);
}

// y_j = v_j R_j z
__device__ inline void res_source(const ResR& R, int j, float vj, float2 z0, float2 z1, float2& y0, float2& y1) {
    const float2 a = cmul(R.r01[j], z1);
    const float2 b = cmulc(z0, R.r01[j]);
    y0 = make_float2(vj * (R.r00[j] * z0.x + a.x), vj * (R.r00[j] * z0.y + a.y));
    y1 = make_float2(vj * (b.x + R.r11[j] * z1.x), vj * (b.y + R.r11[j] * z1.y));
}

__device__ inline void res_accumulate(float (&acc)[16], int j, float2 y0, float2 y1) {
    const float2 c01 = cmulc(y0, y1);
    acc[4 * j + 0] += y0.x * y0.x + y0.y * y0.y;
    acc[4 * j + 1] += y1.x * y1.x + y1.y * y1.y;
    acc[4 * j + 2] += c01.x;
    acc[4 * j + 3] += c01.y;
}

// the workgroup's 16 sums, the same bits in every thread: wave butterfly, then a fixed-order tree over the wave partials
__device__ inline void res_reduce(float (&acc)[16], float (*red)[16], float* tot) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        float v = acc[i];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][i] = v;
    }
    __syncthreads();
    if (threadIdx.x < 16) {
        const int i = threadIdx.x;
        float p[RES_WAVES];
#pragma unroll
        for (int k = 0; k < RES_WAVES; ++k) p[k] = red[k][i];
#pragma unroll
        for (int s = 1; s < RES_WAVES; s <<= 1)
#pragma unroll
            for (int k = 0; k < RES_WAVES; k += 2 * s) p[k] += p[k + s];
        tot[i] = p[0];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = tot[i];
    // (the next write of `red` comes after the second barrier, the next write of `tot` after the next call's first barrier:
    //  every thread has read what it needs by then)
}

// MASKED: the initial estimate is mask * x (Mk: real arena), else Y itself (read before it is overwritten: each thread
// reads and writes only its own frames).  wmax / ext_max: max |x|^2 per (block, group, window) in blockwin order.
template <bool MASKED>
__global__ __launch_bounds__(RES_THREADS) void k_wiener_resident(const float2* __restrict__ X, const float* __restrict__ Mk,
                                                                  float2* Y, const WRow* __restrict__ rows,
                                                                  const int* __restrict__ work, const int* __restrict__ bw_of_work,
                                                                  const float* __restrict__ wmax, const float* __restrict__ ext_max,
                                                                  int Bn, int S, int win_len, int niter) {
    __shared__ float red[RES_WAVES][16];
    __shared__ float tot[16];
    const int row = work[2 * blockIdx.x], w = work[2 * blockIdx.x + 1];
    const WRow r = rows[row];
    const int64_t N = (int64_t)S * r.T;
    const int64_t n0 = (int64_t)w * win_len;
    const int64_t n1 = n0 + win_len < N ? n0 + win_len : N;             // n1 - n0 <= RES_MAX_WINDOW (checked by the host)
    const int bw = bw_of_work[blockIdx.x];
    const float mx2 = ext_max ? fmaxf(wmax[bw], ext_max[bw]) : wmax[bw];
    const float ma = fmaxf(1.f, 0.1f * sqrtf(mx2));                      // norbert :257
    const float inv_ma = 1.f / ma;
    const float2* x0p = X + cidx(r, 2 * Bn, S, r.b * 2, 0);
    const float2* x1p = X + cidx(r, 2 * Bn, S, r.b * 2 + 1, 0);
    const int64_t cstride = (int64_t)r.F * N, jstride = (int64_t)Bn * 2 * cstride;
    const int64_t base = cidx(r, 8 * Bn, S, r.b * 2, 0);                 // target 0, channel 0 of this row (ridx is the same index)
    float2* y00 = Y + base;

    // a frame between iterations: the scaled mix x' = x / ma and the four v_j of the current estimates
    float2 xs0[RES_FPT], xs1[RES_FPT];
    float v[RES_FPT][4];
    float acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
    for (int k = 0; k < RES_FPT; ++k) {
        const int64_t n = n0 + k * RES_THREADS + threadIdx.x;
        xs0[k] = xs1[k] = make_float2(0.f, 0.f);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[k][j] = 0.f;
        if (n < n1) {
            const float2 a = x0p[n], b = x1p[n];
            xs0[k] = make_float2(a.x * inv_ma, a.y * inv_ma);
            xs1[k] = make_float2(b.x * inv_ma, b.y * inv_ma);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float2 y0, y1;
                if (MASKED) {
                    const float m0 = Mk[base + j * jstride + n], m1 = Mk[base + j * jstride + cstride + n];
                    y0 = make_float2(m0 * a.x, m0 * a.y);                // the products the layer-4 epilogue would have stored
                    y1 = make_float2(m1 * b.x, m1 * b.y);
                } else {
                    y0 = y00[j * jstride + n];
                    y1 = y00[j * jstride + cstride + n];
                }
                y0 = make_float2(y0.x * inv_ma, y0.y * inv_ma);
                y1 = make_float2(y1.x * inv_ma, y1.y * inv_ma);
                res_accumulate(acc, j, y0, y1);
                v[k][j] = 0.5f * ((y0.x * y0.x + y0.y * y0.y) + (y1.x * y1.x + y1.y * y1.y));
            }
        }
    }
    res_reduce(acc, red, tot);

    ResR R;
    for (int it = 1; it < niter; ++it) {                                 // iterations 1 .. niter - 1: new v and new sums
        res_R(acc, R);
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
        for (int k = 0; k < RES_FPT; ++k) {
            if (n0 + k * RES_THREADS >= n1) break;                       // uniform over the workgroup
            float2 z0, z1;
            res_solve(R, v[k], xs0[k], xs1[k], z0, z1);                  // (a frame past n1 has x = 0, v = 0: y = 0, adds nothing)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float2 y0, y1;
                res_source(R, j, v[k][j], z0, z1, y0, y1);
                res_accumulate(acc, j, y0, y1);
                v[k][j] = 0.5f * ((y0.x * y0.x + y0.y * y0.y) + (y1.x * y1.x + y1.y * y1.y));
            }
        }
        res_reduce(acc, red, tot);
    }
    res_R(acc, R);                                                        // the last iteration: the estimates, times ma
#pragma unroll
    for (int k = 0; k < RES_FPT; ++k) {
        const int64_t n = n0 + k * RES_THREADS + threadIdx.x;
        if (n < n1) {
            float2 z0, z1;
            res_solve(R, v[k], xs0[k], xs1[k], z0, z1);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float2 y0, y1;
                res_source(R, j, v[k][j], z0, z1, y0, y1);
                y00[j * jstride + n] = make_float2(ma * y0.x, ma * y0.y);
                y00[j * jstride + cstride + n] = make_float2(ma * y1.x, ma * y1.y);
            }
        }
    }
}
