// Framewise and global SDR of a separation against its targets, on the device, gfx950.
//
// The reference scores with museval (xumx_slicq_v2/evaluation.py:16-44) on the host and has `_fast_sdr`
// (xumx_slicq_v2/slicqfinder.py:20-40) for the whole-track ratio.  Here both come from one streaming pass over waveforms that are
// already in HBM.  Definition: a track of N samples has F = max(1, N / W) frames of W samples (one frame
// of N samples when N < W; a tail shorter than W belongs to no frame); per target, row and frame
//   num = sum s^2,   den = sum (s_hat - s)^2,   est = sum s_hat^2        over the frame's samples and both channels,
// differences and products formed in fp64 from the fp32 samples.  Frame value 10 log10(num / den), +inf for den == 0, NaN for a
// silent frame; track scores: the nanmedian of the frame values and 10 log10((sum num + 1e-10) / (sum den + 1e-10)) over all
// cells, the tail included.
//
// Table (device, fp64, zeroed by the caller before a track's first piece): moments (4, B, F + 1, 2) = (num, den), cell F the
// tail beyond the last full frame, followed by the estimates' energies (4, B, F + 1) -- the joint silence rule asks whether an
// ESTIMATE is silent in a frame, which num and den cannot tell (s_hat = 2 s gives den == num as s_hat = 0 does).
//
// Determinism: every cell is cut into slots of SCORE_SEG samples counted from the cell's start.  k_score_moments: one workgroup
// per (slot touched by the piece, row) reduces its samples in a fixed tree (lane-strided sums, wave_sum, four waves in order) and
// STORES 12 partials; k_score_combine: one workgroup per (cell touched, row) sums the cell's partials in a fixed order and adds
// them onto the table, the only writer of that cell in the launch.  No atomics; launches of one stream add in stream order, so
// one way of cutting a track into pieces gives the same bits on every run.
#include "../../include/xumx_slicq_hip.h"
#include "common.h"
#include "prof.h"

namespace xsq {

constexpr int SCORE_SEG = 2048;            // samples of one workgroup: 16 rows x 8 KiB, two 16-byte loads per thread and row
constexpr int SCORE_NM = 12;               // partials per (slot, row): (num, den, est) of the four targets
constexpr int SCORE_MAX_FRAMES = 4096;     // k_score_finalise sorts a track's frames in 32 KiB of LDS

struct ScoreGeom {
    int64_t frames, flen, N;               // F; samples of a frame (W, or N when N < W); samples of the track
    int64_t spf;                           // slots per cell: ceil(flen / SCORE_SEG)
};

static inline ScoreGeom score_geom(int64_t N, int64_t W) {
    ScoreGeom g;
    g.N = N;
    g.frames = N / W > 1 ? N / W : 1;
    g.flen = N < W ? N : W;
    g.spf = (g.flen + SCORE_SEG - 1) / SCORE_SEG;
    return g;
}
// the global slot that holds absolute sample k
static inline int64_t score_slot_of(const ScoreGeom& g, int64_t k) {
    const int64_t cell = k / g.flen < g.frames ? k / g.flen : g.frames;
    return cell * g.spf + (k - cell * g.flen) / SCORE_SEG;
}

struct ScoreArgs {
    const float* est; const float* tgt;    // sample `offset` of row 0
    int perm[4];                           // stem of est that estimates target i
    int B;
    int64_t n, es, ts, offset;             // samples of the piece, row strides, first sample of the piece in the track
    ScoreGeom g;
    int64_t slot0;                         // global slot of blockIdx.x == 0
    int vec, phase;                        // vec: every row may be read 16 bytes at a time from samples k with (phase + k) % 4 == 0
};

struct ScoreAcc {
    double a[SCORE_NM];
    __device__ __forceinline__ void add(int i, float ev, float tv) {
        const double e = (double)ev, t = (double)tv, d = e - t;
        a[3 * i] += t * t;
        a[3 * i + 1] += d * d;
        a[3 * i + 2] += e * e;
    }
};

// grid (slots touched by the piece, B).  partial: [row][blockIdx.x][12].
__global__ __launch_bounds__(256) void k_score_moments(ScoreArgs A, double* __restrict__ partial) {
    const int b = blockIdx.y, tid = threadIdx.x;
    const int64_t slot = A.slot0 + blockIdx.x;
    const int64_t cell = slot / A.g.spf;
    const int64_t cell_lo = cell * A.g.flen, cell_hi = cell < A.g.frames ? cell_lo + A.g.flen : A.g.N;
    int64_t lo = cell_lo + (slot - cell * A.g.spf) * SCORE_SEG, hi = lo + SCORE_SEG < cell_hi ? lo + SCORE_SEG : cell_hi;
    lo = (lo > A.offset ? lo : A.offset) - A.offset;                     // relative to the piece from here on
    hi = (hi < A.offset + A.n ? hi : A.offset + A.n) - A.offset;
    const float* pe[8];
    const float* pt[8];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            pe[2 * i + c] = A.est + (((int64_t)A.perm[i] * A.B + b) * 2 + c) * A.es;
            pt[2 * i + c] = A.tgt + (((int64_t)i * A.B + b) * 2 + c) * A.ts;
        }
    ScoreAcc acc;
#pragma unroll
    for (int m = 0; m < SCORE_NM; ++m) acc.a[m] = 0.0;
    if (A.vec) {
        int64_t ka = lo + ((4 - (int)((A.phase + lo) & 3)) & 3);         // first 16-byte boundary of the rows
        if (ka > hi) ka = hi;
        const int64_t nv = (hi - ka) >> 2, kb = ka + 4 * nv;
        for (int64_t v = tid; v < nv; v += 256) {
            const int64_t k = ka + 4 * v;
            float4 e[8], t[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                e[r] = *reinterpret_cast<const float4*>(pe[r] + k);
                t[r] = *reinterpret_cast<const float4*>(pt[r] + k);
            }
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                acc.add(r >> 1, e[r].x, t[r].x);
                acc.add(r >> 1, e[r].y, t[r].y);
                acc.add(r >> 1, e[r].z, t[r].z);
                acc.add(r >> 1, e[r].w, t[r].w);
            }
        }
        const int head = (int)(ka - lo), edge = head + (int)(hi - kb);    // at most 3 + 3 samples beside the 16-byte groups
        if (tid < edge) {
            const int64_t k = tid < head ? lo + tid : kb + (tid - head);
#pragma unroll
            for (int r = 0; r < 8; ++r) acc.add(r >> 1, pe[r][k], pt[r][k]);
        }
    } else {
        for (int64_t k = lo + tid; k < hi; k += 256) {
            float e[8], t[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) { e[r] = pe[r][k]; t[r] = pt[r][k]; }
#pragma unroll
            for (int r = 0; r < 8; ++r) acc.add(r >> 1, e[r], t[r]);
        }
    }
    __shared__ double red[4][SCORE_NM];
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int m = 0; m < SCORE_NM; ++m) {
        const double v = wave_sum(acc.a[m]);
        if (lane == 0) red[wave][m] = v;
    }
    __syncthreads();
    if (tid < SCORE_NM)
        partial[((int64_t)b * gridDim.x + blockIdx.x) * SCORE_NM + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// grid (cells touched by the piece, B), 256 threads = 16 groups of 16 lanes: lane m < 12 of group q sums partial m of the
// cell's slots q, q + 16, ...; thread m < 12 then sums the 16 groups in order and adds onto the table.
__global__ __launch_bounds__(256) void k_score_combine(const double* __restrict__ partial, int64_t nslots, ScoreGeom g, int B,
                                                        int64_t slot0, int64_t slot1, int64_t cell0, double* __restrict__ table) {
    const int b = blockIdx.y, tid = threadIdx.x, m = tid & 15, q = tid >> 4;
    const int64_t cell = cell0 + blockIdx.x;
    const int64_t s0 = (cell * g.spf > slot0 ? cell * g.spf : slot0) - slot0;
    const int64_t s1 = (cell * g.spf + g.spf - 1 < slot1 ? cell * g.spf + g.spf - 1 : slot1) - slot0;
    __shared__ double red[16][SCORE_NM];
    if (m < SCORE_NM) {
        double a = 0.0;
        for (int64_t s = s0 + q; s <= s1; s += 16) a += partial[((int64_t)b * nslots + s) * SCORE_NM + m];
        red[q][m] = a;
    }
    __syncthreads();
    if (tid < SCORE_NM) {
        double a = red[0][tid];
#pragma unroll
        for (int k = 1; k < 16; ++k) a += red[k][tid];
        const int i = tid / 3, j = tid - 3 * i;
        const int64_t cells = g.frames + 1, at = ((int64_t)i * B + b) * cells + cell;
        double* dst = j < 2 ? table + at * 2 + j : table + 4 * (int64_t)B * cells * 2 + at;
        *dst += a;
    }
}

// doubles as 64-bit keys in their numeric order, -inf first and +inf last; NaN (a silent frame, or padding) behind them all
constexpr unsigned long long SCORE_KEY_NAN = ~0ull;
__device__ __forceinline__ unsigned long long score_key(double v) {
    if (v != v) return SCORE_KEY_NAN;
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : u | 0x8000000000000000ull;
}
__device__ __forceinline__ double score_unkey(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? k & 0x7fffffffffffffffull : ~k));
}

// grid (4, B): the frame values of one (target, row), their nanmedian by a bitonic sort of P = 2^p >= F keys in LDS, and
// the global ratio.  silent_mode 0: a frame is silent when ANY target's reference or estimate has no energy in it; 1: the
// target's OWN reference.
__global__ __launch_bounds__(256) void k_score_finalise(const double* __restrict__ table, int B, int F, int P, int silent_mode,
                                                         double* __restrict__ out_frames, double* __restrict__ out_scores) {
    const int i = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int64_t cells = (int64_t)F + 1;
    const double* est = table + 4 * (int64_t)B * cells * 2;
    const double nan = __longlong_as_double(0x7ff8000000000000ll), inf = __longlong_as_double(0x7ff0000000000000ll);
    __shared__ unsigned long long keys[SCORE_MAX_FRAMES];
    __shared__ double red[4][2];
    __shared__ int valid;
    if (tid == 0) valid = 0;
    double snum = 0.0, sden = 0.0;
    for (int f = tid; f < P; f += 256) {
        unsigned long long key = SCORE_KEY_NAN;
        if (f < F) {
            const int64_t at = ((int64_t)i * B + b) * cells + f;
            const double num = table[at * 2], den = table[at * 2 + 1];
            bool silent = num == 0.0;
            if (silent_mode == 0)
                for (int j = 0; j < 4; ++j) {
                    const int64_t aj = ((int64_t)j * B + b) * cells + f;
                    silent = silent || table[aj * 2] == 0.0 || est[aj] == 0.0;
                }
            const double v = silent ? nan : den == 0.0 ? inf : 10.0 * log10(num / den);
            out_frames[((int64_t)i * B + b) * F + f] = v;
            key = score_key(v);
            snum += num;
            sden += den;
        }
        keys[f] = key;
    }
    if (tid == 0) {                                                       // the tail cell counts in the global ratio only
        const int64_t at = ((int64_t)i * B + b) * cells + F;
        snum += table[at * 2];
        sden += table[at * 2 + 1];
    }
    snum = wave_sum(snum);
    sden = wave_sum(sden);
    if ((tid & 63) == 0) { red[tid >> 6][0] = snum; red[tid >> 6][1] = sden; }
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int x = tid; x < P; x += 256) {
                const int y = x ^ j;
                if (y > x) {
                    const unsigned long long u = keys[x], w = keys[y];
                    if ((u > w) == ((x & k) == 0)) { keys[x] = w; keys[y] = u; }
                }
            }
            __syncthreads();
        }
    for (int x = tid; x < P; x += 256)                                     // one x at most: the last key that is no NaN
        if (keys[x] != SCORE_KEY_NAN && (x + 1 == P || keys[x + 1] == SCORE_KEY_NAN)) valid = x + 1;
    __syncthreads();
    if (tid == 0) {
        const int n = valid;
        double med = nan;
        if (n > 0) med = (n & 1) ? score_unkey(keys[n / 2]) : (score_unkey(keys[n / 2 - 1]) + score_unkey(keys[n / 2])) * 0.5;
        const double tn = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0], td = ((red[0][1] + red[1][1]) + red[2][1]) + red[3][1];
        out_scores[((int64_t)i * B + b) * 2] = med;
        out_scores[((int64_t)i * B + b) * 2 + 1] = 10.0 * log10((tn + 1e-10) / (td + 1e-10));
    }
}

static int score_shape_ok(const char* who, int B, int64_t N, int64_t W) {
    XSQ_REQUIRE(B > 0 && B <= 65535 && N > 0 && W > 0, "%s: B=%d N=%lld W=%lld (1 <= B <= 65535, N >= 1, W >= 1)", who, B, (long long)N,
                (long long)W);
    const ScoreGeom g = score_geom(N, W);
    XSQ_REQUIRE(g.frames <= SCORE_MAX_FRAMES, "%s: %lld frames of %lld samples; the median is a sort in LDS and holds at most %d frames",
                who, (long long)g.frames, (long long)W, SCORE_MAX_FRAMES);
    XSQ_REQUIRE((g.frames + 1) * g.spf <= 0x7fffffff, "%s: N=%lld W=%lld is more than 2^31 slots of %d samples", who, (long long)N,
                (long long)W, SCORE_SEG);
    return XSQ_OK;
}

}  // namespace xsq

using namespace xsq;

extern "C" {

int xsq_score_max_frames(void) { return SCORE_MAX_FRAMES; }

int xsq_score_workspace(int B, int64_t N, int64_t W, size_t* table_bytes, size_t* ws_bytes) {
    XSQ_REQUIRE(table_bytes && ws_bytes, "xsq_score_workspace: null argument");
    *table_bytes = *ws_bytes = 0;
    if (int rc = score_shape_ok("xsq_score_workspace", B, N, W)) return rc;
    const ScoreGeom g = score_geom(N, W);
    *table_bytes = (size_t)4 * B * (g.frames + 1) * 3 * 8;
    *ws_bytes = al256((size_t)B * (g.frames + 1) * g.spf * SCORE_NM * 8);
    return XSQ_OK;
}

int xsq_score_accumulate(const float* est, const float* tgt, const int* perm, int B, int64_t n, int64_t est_row_stride,
                         int64_t tgt_row_stride, int64_t offset, int64_t N, int64_t W, double* table, void* ws, size_t ws_bytes,
                         void* stream_) {
    const char* who = "xsq_score_accumulate";
    XSQ_REQUIRE(est && tgt && perm && table && ws, "%s: null argument", who);
    if (int rc = score_shape_ok(who, B, N, W)) return rc;
    XSQ_REQUIRE(n > 0 && offset >= 0 && offset <= N - n, "%s: piece [%lld, +%lld) of a track of %lld samples", who, (long long)offset,
                (long long)n, (long long)N);
    XSQ_REQUIRE(est_row_stride >= n && tgt_row_stride >= n, "%s: row strides %lld / %lld below the piece's %lld samples", who,
                (long long)est_row_stride, (long long)tgt_row_stride, (long long)n);
    int seen = 0;
    for (int i = 0; i < 4; ++i) {
        XSQ_REQUIRE(perm[i] >= 0 && perm[i] < 5 && !(seen >> perm[i] & 1), "%s: perm = %d %d %d %d is no choice of four different stems out of 0..4",
                    who, perm[0], perm[1], perm[2], perm[3]);
        seen |= 1 << perm[i];
    }
    ScoreArgs A;
    A.est = est; A.tgt = tgt; A.B = B; A.n = n; A.es = est_row_stride; A.ts = tgt_row_stride; A.offset = offset;
    for (int i = 0; i < 4; ++i) A.perm[i] = perm[i];
    A.g = score_geom(N, W);
    const int64_t slot0 = score_slot_of(A.g, offset), slot1 = score_slot_of(A.g, offset + n - 1), nslots = slot1 - slot0 + 1;
    const int64_t cell0 = slot0 / A.g.spf, cell1 = slot1 / A.g.spf;
    XSQ_REQUIRE(ws_bytes >= (size_t)B * nslots * SCORE_NM * 8, "%s: workspace too small (%zu needed, %zu given)", who,
                (size_t)B * nslots * SCORE_NM * 8, ws_bytes);
    A.slot0 = slot0;
    const uintptr_t ea = (uintptr_t)est, ta = (uintptr_t)tgt;
    // with row strides that are multiples of 4 floats, sample k of EVERY row starts 16 bytes where (phase + k) % 4 == 0 -- if
    // the two tensors agree on the phase; otherwise (a piece cut at an odd sample of a contiguous tensor) 4-byte loads
    A.phase = (int)((ea >> 2) & 3);
    A.vec = (ea & 3) == 0 && (ta & 3) == 0 && ((ta >> 2) & 3) == (uintptr_t)A.phase && est_row_stride % 4 == 0 && tgt_row_stride % 4 == 0;
    hipStream_t stream = (hipStream_t)stream_;
    { XSQ_PROF("score_moments", stream);
      hipLaunchKernelGGL(k_score_moments, dim3((unsigned)nslots, B), dim3(256), 0, stream, A, (double*)ws); }
    { XSQ_PROF("score_combine", stream);
      hipLaunchKernelGGL(k_score_combine, dim3((unsigned)(cell1 - cell0 + 1), B), dim3(256), 0, stream, (const double*)ws, nslots, A.g, B,
                         slot0, slot1, cell0, table); }
    XSQ_HIP(hipGetLastError());
    return XSQ_OK;
}

int xsq_score_finalise(const double* table, int B, int64_t frames, int silent_mode, double* out_frames, double* out_scores, void* stream_) {
    const char* who = "xsq_score_finalise";
    XSQ_REQUIRE(table && out_frames && out_scores, "%s: null argument", who);
    XSQ_REQUIRE(B > 0 && B <= 65535 && frames > 0, "%s: B=%d frames=%lld", who, B, (long long)frames);
    XSQ_REQUIRE(frames <= SCORE_MAX_FRAMES, "%s: %lld frames; the median is a sort in LDS and holds at most %d frames", who,
                (long long)frames, SCORE_MAX_FRAMES);
    XSQ_REQUIRE(silent_mode == XSQ_SCORE_SILENT_ANY || silent_mode == XSQ_SCORE_SILENT_OWN, "%s: silent_mode %d (0 = any, 1 = own)", who,
                silent_mode);
    int P = 1;
    while (P < frames) P <<= 1;
    hipStream_t stream = (hipStream_t)stream_;
    { XSQ_PROF("score_finalise", stream);
      hipLaunchKernelGGL(k_score_finalise, dim3(4, B), dim3(256), 0, stream, table, B, (int)frames, P, silent_mode, out_frames, out_scores); }
    XSQ_HIP(hipGetLastError());
    return XSQ_OK;
}

}  // extern "C"
