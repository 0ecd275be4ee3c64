// Placement of packed stems into their tracks: the "final waveform concat" of the sharded path, gfx950.
//
// Reference: xumx_slicq_v2/separator.py:229-231 -- every chunk's (4, nb_samples, 2, n) estimate is appended to a
// list and the list is joined by a hard torch.cat along the sample axis.  On one GPU the inverse transform writes
// its rows straight into the result (xsq_slicqt_inverse_rows).  With the chunk items sharded over the ranks the
// stems of the OTHER ranks arrive packed in an all-gather buffer; one launch of k_place_rows moves every row
// (item, target, sample, channel) of a round to its span of the per-track tensors: an HBM copy driven by a row
// table, 16-byte accesses wherever source and destination share their alignment.
// k_crossfade_place is the other join, of Separator.forward_overlapped: the segments of a pass overlap and are blended
// with linear fades while they are placed (cadenza/enhance.py:35-99).
#include "../../include/xumx_slicq_hip.h"
#include "common.h"
#include "prof.h"

namespace xsq {

constexpr int PLACE_THREADS = 256;
constexpr int PLACE_VEC_PER_THREAD = 8;                                   // float4 per thread and grid-x step
constexpr int64_t PLACE_SPAN = (int64_t)PLACE_THREADS * PLACE_VEC_PER_THREAD * 4;   // floats per workgroup

// table: nrows x (src offset, dst offset, length), all in floats.
__global__ __launch_bounds__(PLACE_THREADS) void k_place_rows(const float* __restrict__ src, float* __restrict__ dst,
                                                               const int64_t* __restrict__ table) {
    const int64_t so = table[3 * blockIdx.y], dof = table[3 * blockIdx.y + 1], len = table[3 * blockIdx.y + 2];
    const int64_t first = (int64_t)blockIdx.x * PLACE_SPAN;
    if (first >= len) return;
    const float* s = src + so;
    float* d = dst + dof;
    // floats in front of the first 16-byte boundary of the DESTINATION row (same for the source when the two
    // offsets agree modulo 4, the common case: chunk and track lengths are multiples of 4 except odd-length tracks)
    const int head = (int)((4 - (dof & 3)) & 3);
    const bool same = ((so ^ dof) & 3) == 0;
    if (same) {
        const int64_t nvec = len > head ? (len - head) >> 2 : 0;
        if (blockIdx.x == 0) {                                // the row's ragged ends: < 4 floats on either side
            const int64_t t = threadIdx.x, tail = head + 4 * nvec + t;
            if (t < head && t < len) d[t] = s[t];
            if (t < 3 && tail >= head && tail < len) d[tail] = s[tail];
        }
        const float4* s4 = reinterpret_cast<const float4*>(s + head);
        float4* d4 = reinterpret_cast<float4*>(d + head);
        const int64_t v0 = (int64_t)blockIdx.x * (PLACE_THREADS * PLACE_VEC_PER_THREAD) + threadIdx.x;
        float4 r[PLACE_VEC_PER_THREAD];
#pragma unroll
        for (int i = 0; i < PLACE_VEC_PER_THREAD; ++i) {
            const int64_t v = v0 + (int64_t)i * PLACE_THREADS;
            if (v < nvec) r[i] = s4[v];
        }
#pragma unroll
        for (int i = 0; i < PLACE_VEC_PER_THREAD; ++i) {
            const int64_t v = v0 + (int64_t)i * PLACE_THREADS;
            if (v < nvec) d4[v] = r[i];
        }
    } else {                                                  // rows of different alignment: 4-byte path
        const int64_t end = first + PLACE_SPAN < len ? first + PLACE_SPAN : len;
        for (int64_t i = first + threadIdx.x; i < end; i += PLACE_THREADS) d[i] = s[i];
    }
}

// ---- overlapped segments (Separator.forward_overlapped): cadenza/enhance.py:35-99 (separate_sources) by placement.
// The un-faded stems of the k equal-length segments of one pass lie in a scratch arena (row (target, segment * nb + b, c)
// at rows[...], n samples each); segment j covers samples [start + j * stride, + n) of the track and shares its first
// ov = n - stride samples with the tail of segment j - 1.  One thread per FOUR output samples of one (target, b, c) row,
// aligned to the destination (segment starts are arbitrary and mostly odd: the sources are read 4 bytes at a time, the
// destination is written 16 bytes at a time).  Each sample finds its segment and, inside a fade, the previous one:
//     out = fl(fl(w_out * a) + fl(w_in * b)),  w_in = i / (ov - 1),  w_out = (ov - 1 - i) / (ov - 1)   (torchaudio Fade, linear)
// The head of the pass's FIRST segment fades against a segment of the previous pass, whose launch -- earlier on the same
// stream -- stored fl(w_out * a) there: fl(w_in * b) is added onto it.  No contraction, so both routes give the same bits.
struct CrossfadeArgs {
    const float* src;
    const int64_t* rows;      // [2J * k * nb] scratch row offsets, (target, segment * nb + b, c)
    float* dst;               // (J, nb, 2, N)
    int64_t N, start;
    int nb, k, ov, fade_in_first, fade_out_last;
    unsigned stride, n, range;      // range = (k - 1) * stride + n < 2^31
};

__device__ __forceinline__ float crossfade_sample(const CrossfadeArgs& A, const float* d, int t, int bc, unsigned u) {
#pragma clang fp contract(off)
    const unsigned j = min(u / A.stride, (unsigned)(A.k - 1));
    const unsigned i = u - j * A.stride;
    const int64_t r = ((int64_t)t * A.k * A.nb + (int64_t)j * A.nb) * 2 + bc;
    const float b = A.src[A.rows[r] + i];
    const float den = (float)(A.ov - 1);
    if (i < (unsigned)A.ov && (j > 0 || A.fade_in_first)) {    // head of segment j
        const float w_in = A.ov > 1 ? (float)i / den : 0.f;
        if (j == 0) return d[u] + w_in * b;                    // the previous pass left fl(w_out * a) here
        const float w_out = A.ov > 1 ? (float)(A.ov - 1 - (int)i) / den : 1.f;
        const float a = A.src[A.rows[r - 2 * A.nb] + i + A.stride];
        return w_out * a + w_in * b;
    }
    if (A.fade_out_last && j == (unsigned)(A.k - 1) && i >= A.n - (unsigned)A.ov) {     // tail the next pass fades against
        const int q = (int)(i - (A.n - (unsigned)A.ov));
        const float w_out = A.ov > 1 ? (float)(A.ov - 1 - q) / den : 1.f;
        return w_out * b;
    }
    return b;
}

__global__ __launch_bounds__(PLACE_THREADS) void k_crossfade_place(const CrossfadeArgs A) {
    const int row = blockIdx.y;                                // (target, b, c) of the result
    const int t = row / (2 * A.nb), bc = row - t * 2 * A.nb;
    float* d = A.dst + (int64_t)row * A.N + A.start;
    const int lead = (int)((reinterpret_cast<uintptr_t>(d) >> 2) & 3);      // floats behind the last 16-byte boundary
    const int64_t u0 = ((int64_t)blockIdx.x * PLACE_THREADS + threadIdx.x) * 4 - lead;
    if (u0 >= (int64_t)A.range) return;
    if (u0 >= 0 && u0 + 4 <= (int64_t)A.range) {
        float4 v;
        v.x = crossfade_sample(A, d, t, bc, (unsigned)u0);
        v.y = crossfade_sample(A, d, t, bc, (unsigned)u0 + 1);
        v.z = crossfade_sample(A, d, t, bc, (unsigned)u0 + 2);
        v.w = crossfade_sample(A, d, t, bc, (unsigned)u0 + 3);
        *reinterpret_cast<float4*>(d + u0) = v;
        return;
    }
    for (int e = 0; e < 4; ++e) {                              // the ragged ends of the covered range
        const int64_t u = u0 + e;
        if (u >= 0 && u < (int64_t)A.range) d[u] = crossfade_sample(A, d, t, bc, (unsigned)u);
    }
}

}  // namespace xsq

using namespace xsq;

extern "C" int xsq_place_rows(const float* src, float* dst, const int64_t* table, int nrows, int64_t max_len,
                              void* stream) {
    XSQ_REQUIRE(src && dst && table, "xsq_place_rows: null pointer");
    XSQ_REQUIRE(nrows >= 0 && nrows <= 65535 && max_len >= 0, "xsq_place_rows: nrows %d (<= 65535), max_len %lld", nrows,
                (long long)max_len);
    if (nrows == 0 || max_len == 0) return XSQ_OK;
    hipStream_t st = (hipStream_t)stream;
    const int64_t gx = (max_len + PLACE_SPAN - 1) / PLACE_SPAN;
    XSQ_REQUIRE(gx < (1ll << 31), "xsq_place_rows: max_len too large");
    XSQ_PROF("place_rows", st);
    hipLaunchKernelGGL(k_place_rows, dim3((unsigned)gx, (unsigned)nrows), dim3(PLACE_THREADS), 0, st, src, dst, table);
    XSQ_HIP(hipGetLastError());
    return XSQ_OK;
}

extern "C" int xsq_crossfade_place(const float* scratch, const int64_t* row_offsets, float* dst, int nb, int64_t N, int64_t start,
                                   int64_t stride, int64_t n, int k, int ov, int fade_in_first, int fade_out_last, void* stream) {
    return xsq_crossfade_place_sources(scratch, row_offsets, dst, 4, nb, N, start, stride, n, k, ov, fade_in_first, fade_out_last, stream);
}

extern "C" int xsq_crossfade_place_sources(const float* scratch, const int64_t* row_offsets, float* dst, int nsources, int nb, int64_t N,
                                           int64_t start, int64_t stride, int64_t n, int k, int ov, int fade_in_first, int fade_out_last,
                                           void* stream) {
    XSQ_REQUIRE(scratch && row_offsets && dst, "xsq_crossfade_place: null pointer");
    XSQ_REQUIRE(nsources == 4 || nsources == 5, "xsq_crossfade_place: %d sources (4, or 5 with the residual)", nsources);
    XSQ_REQUIRE(nb >= 1 && 2 * nsources * (int64_t)nb <= 65535 && N >= 1 && start >= 0 && n >= 1 && k >= 1,
                "xsq_crossfade_place: nb=%d N=%lld start=%lld n=%lld k=%d", nb, (long long)N, (long long)start, (long long)n, k);
    XSQ_REQUIRE(ov >= 0 && ov < (1 << 24) && ov <= n, "xsq_crossfade_place: ov=%d (0 .. min(n, 2^24 - 1))", ov);
    if (k == 1) stride = n;
    // consecutive segments share exactly ov samples and segments two apart none: a sample has one or two terms
    XSQ_REQUIRE(k == 1 || (stride >= 1 && n - stride == ov && stride >= ov),
                "xsq_crossfade_place: k=%d segments of n=%lld at stride=%lld do not overlap by ov=%d alone", k, (long long)n, (long long)stride, ov);
    XSQ_REQUIRE(!(fade_in_first && fade_out_last) || 2 * (int64_t)ov <= n, "xsq_crossfade_place: n=%lld is shorter than the two fades of ov=%d", (long long)n, ov);
    const int64_t range = (int64_t)(k - 1) * stride + n;
    XSQ_REQUIRE(range < (1ll << 31) - 8 && start + range <= N, "xsq_crossfade_place: the pass covers [%lld, %lld) of N=%lld (< 2^31 samples per launch)",
                (long long)start, (long long)(start + range), (long long)N);
    CrossfadeArgs A;
    A.src = scratch; A.rows = row_offsets; A.dst = dst; A.N = N; A.start = start;
    A.nb = nb; A.k = k; A.ov = ov; A.fade_in_first = (fade_in_first && ov > 0) ? 1 : 0; A.fade_out_last = (fade_out_last && ov > 0) ? 1 : 0;
    A.stride = (unsigned)stride; A.n = (unsigned)n; A.range = (unsigned)range;
    hipStream_t st = (hipStream_t)stream;
    const int64_t gx = (range + 3 + 4 * PLACE_THREADS - 1) / (4 * PLACE_THREADS);       // + 3: the destination's lead-in
    XSQ_PROF("crossfade_place", st);
    hipLaunchKernelGGL(k_crossfade_place, dim3((unsigned)gx, (unsigned)(2 * nsources * nb)), dim3(PLACE_THREADS), 0, st, A);
    XSQ_HIP(hipGetLastError());
    return XSQ_OK;
}
