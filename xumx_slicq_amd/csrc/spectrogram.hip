// The sliCQT spectrogram on the device, gfx950: overlap-add of the slices, magnitude in dB, exact order statistics for
// the colour scale, and the raster that leaves the device.
//
// The reference (xumx_slicq_v2/visualization.py:13-35, :55-81) overlap-adds in a Python loop, takes torch.quantile of a whole
// block and hands every coefficient to matplotlib.  Here the coefficients are read where the forward transform left them:
//   k_spec_ola     complex arena -> complex rows, what overlap_add_slicq returns (both `flatten` settings)
//   k_spec_db      arena -> (B, F_b, N_b) fp32 per block in ONE pass: overlap-add, magnitude, log, channel mean, crop and
//                  truncation; every contributing coefficient is read once, 16 bytes at a time (a half-slice is a whole number
//                  of float4 because T_b % 4 == 0); no complex intermediate is written
//   k_spec_hist / k_spec_pick   radix select (4 passes of 8 bits) over the order-preserving integer image of the floats,
//                  -inf included: histograms in LDS, combined with INTEGER atomics only, both ranks selected together
//   k_spec_raster  image (B, nbands, W): pixel (row f of block b, column w) = max of the block's dB columns [lo, hi)
// No floating-point atomic anywhere in this file: every output has the same bits on every run.
//
// Geometry goes to the kernels by value (SpecGeom, at most SPEC_MAX_BLOCKS blocks): blockIdx.y is a band of the plan and the
// workgroup walks the block list to its block -- a scalar loop of at most nblocks steps in front of kilobytes of streaming.
#include "../../include/xumx_slicq_hip.h"
#include "common.h"
#include "prof.h"

namespace xsq {

constexpr int SPEC_MAX_BLOCKS = 128;
constexpr int SPEC_PAIRS = 4;                       // 16-byte groups (two complex points) per thread and operand
constexpr int SPEC_CHUNK = 256 * 2 * SPEC_PAIRS;    // points of one workgroup
constexpr int SPEC_HIST_CHUNK = 256 * 16;           // values of one histogram workgroup
constexpr int SPEC_RASTER_REP = 8;                  // pixel groups of one raster workgroup, one after the other

struct SpecGeom {
    int nblocks, B, S;                              // B: batch items (two channels each); k_spec_ola: packed channels
    int F[SPEC_MAX_BLOCKS], T[SPEC_MAX_BLOCKS], N[SPEC_MAX_BLOCKS];
};

// where band `g` of the plan lives: its block, its row there, and the sums over the earlier blocks
struct SpecAt { int k, f; int64_t cum, out; };      // cum: sum F*T; out: sum F*N
__device__ __forceinline__ SpecAt spec_locate(const SpecGeom& G, int g) {
    SpecAt a{0, g, 0, 0};
    while (a.f >= G.F[a.k]) {
        a.f -= G.F[a.k];
        a.cum += (int64_t)G.F[a.k] * G.T[a.k];
        a.out += (int64_t)G.F[a.k] * G.N[a.k];
        ++a.k;
    }
    return a;
}

// THE dB value of one point from its two channels: 20 log10 |c| per channel (hypotf: no overflow or underflow through
// squaring; |0| gives -inf), then the mean of the two dB values -- log first, mix-down second, as the reference.  Every
// kernel that forms a dB value calls this, with contraction off, so all of them give the same bits.
__device__ __forceinline__ float spec_db(float re0, float im0, float re1, float im1) {
#pragma clang fp contract(off)
    const float d0 = 20.0f * log10f(hypotf(re0, im0));
    const float d1 = 20.0f * log10f(hypotf(re1, im1));
    return (d0 + d1) * 0.5f;
}

// grid (chunks of the longest row, bands, B).  Point p of a row: overlap-add position p + h (h = T/2 columns are dropped at
// each end), which lies in the second half of slice j = p / h and the first half of slice j + 1 -- exactly two contributions
// at every point kept; flatten: position p + h of the slices side by side.
template <bool FLAT>
__global__ __launch_bounds__(256) void k_spec_db(SpecGeom G, const float* __restrict__ arena, float* __restrict__ out) {
    const SpecAt at = spec_locate(G, blockIdx.y);
    const int F = G.F[at.k], T = G.T[at.k], N = G.N[at.k], h = T >> 1, S = G.S, b = blockIdx.z;
    const int p0 = blockIdx.x * SPEC_CHUNK;
    if (p0 >= N) return;
    const float* blk = arena + 4 * (int64_t)G.B * S * at.cum;
    const float* x0 = blk + (((int64_t)(2 * b) * F + at.f) * S) * T * 2;
    const float* x1 = blk + (((int64_t)(2 * b + 1) * F + at.f) * S) * T * 2;
    float* o = out + (int64_t)G.B * at.out + ((int64_t)b * F + at.f) * N;
    float4 a0[SPEC_PAIRS], a1[SPEC_PAIRS], b0[SPEC_PAIRS], b1[SPEC_PAIRS];
    int p[SPEC_PAIRS];
#pragma unroll
    for (int u = 0; u < SPEC_PAIRS; ++u) {
        p[u] = p0 + 2 * ((int)threadIdx.x + 256 * u);
        if (p[u] < N) {                              // p even, h even: the pair never straddles a half-slice, and p + 1 is a
            int64_t i;                               // valid position of the row even when N is odd (N < (S - 1) h then)
            if (FLAT) i = (int64_t)p[u] + h;
            else { const int j = p[u] / h; i = (int64_t)j * T + h + (p[u] - j * h); }
            a0[u] = *reinterpret_cast<const float4*>(x0 + 2 * i);
            a1[u] = *reinterpret_cast<const float4*>(x1 + 2 * i);
            if (!FLAT) {
                b0[u] = *reinterpret_cast<const float4*>(x0 + 2 * (i + h));
                b1[u] = *reinterpret_cast<const float4*>(x1 + 2 * (i + h));
            }
        }
    }
#pragma unroll
    for (int u = 0; u < SPEC_PAIRS; ++u)
        if (p[u] < N) {
            float4 c0 = a0[u], c1 = a1[u];
            if (!FLAT) {
                c0.x += b0[u].x; c0.y += b0[u].y; c0.z += b0[u].z; c0.w += b0[u].w;
                c1.x += b1[u].x; c1.y += b1[u].y; c1.z += b1[u].z; c1.w += b1[u].w;
            }
            o[p[u]] = spec_db(c0.x, c0.y, c1.x, c1.y);
            if (p[u] + 1 < N) o[p[u] + 1] = spec_db(c0.z, c0.w, c1.z, c1.w);
        }
}

// grid (chunks of the longest row, bands, packed channels).  Row of Lout = (S + 1) h complex points (flatten: S T): point p
// in segment j = p / h is 0 + x[j - 1, h + r] + x[j, r], the reference's zero-initialised `out[ptr : ptr + T] += slice i` for
// i ascending -- one correctly rounded fp32 add per component wherever two slices meet.
template <bool FLAT>
__global__ __launch_bounds__(256) void k_spec_ola(SpecGeom G, const float* __restrict__ arena, float* __restrict__ out) {
    const SpecAt at = spec_locate(G, blockIdx.y);
    const int F = G.F[at.k], T = G.T[at.k], h = T >> 1, S = G.S, c = blockIdx.z;
    const int64_t Lout = FLAT ? (int64_t)S * T : (int64_t)(S + 1) * h;
    const int64_t p0 = (int64_t)blockIdx.x * SPEC_CHUNK;
    if (p0 >= Lout) return;
    const float* x = arena + 2 * (int64_t)G.B * S * at.cum + (((int64_t)c * F + at.f) * S) * T * 2;
    // earlier blocks hold F_b * Lout_b points per channel: FLAT S * cum, else (S + 1) * cum / 2 (T even)
    const int64_t before = FLAT ? (int64_t)S * at.cum : (int64_t)(S + 1) * (at.cum >> 1);
    float* o = out + 2 * ((int64_t)G.B * before + ((int64_t)c * F + at.f) * Lout);
#pragma unroll
    for (int u = 0; u < SPEC_PAIRS; ++u) {
        const int64_t p = p0 + 2 * ((int64_t)threadIdx.x + 256 * u);
        if (p >= Lout) continue;
        float4 v;
        if (FLAT) v = *reinterpret_cast<const float4*>(x + 2 * p);
        else {
            const int j = (int)(p / h), r = (int)(p - (int64_t)j * h);
            v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (j >= 1) {
                const float4 a = *reinterpret_cast<const float4*>(x + 2 * ((int64_t)(j - 1) * T + h + r));
                v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w;
            }
            if (j < S) {
                const float4 a = *reinterpret_cast<const float4*>(x + 2 * ((int64_t)j * T + r));
                v.x += a.x; v.y += a.y; v.z += a.z; v.w += a.w;
            }
        }
        *reinterpret_cast<float4*>(o + 2 * p) = v;
    }
}

// ---- exact order statistics -------------------------------------------------------------------------------------------
// fp32 values as 32-bit keys in their numeric order: -inf first, +inf last (NaNs, which the dB pass does not produce from
// finite coefficients, sort by their sign beyond the infinities).
__device__ __forceinline__ unsigned spec_key(float v) {
    const unsigned u = __builtin_bit_cast(unsigned, v);
    return (u >> 31) ? ~u : u | 0x80000000u;
}
__device__ __forceinline__ float spec_unkey(unsigned k) { return __builtin_bit_cast(float, (k >> 31) ? k & 0x7fffffffu : ~k); }

struct SpecSel { unsigned prefix[2], rank[2]; };    // per batch item: key bits found so far, rank left among the keys sharing them

__global__ __launch_bounds__(256) void k_spec_sel_init(SpecSel* __restrict__ st, unsigned* __restrict__ hist, unsigned k_lo, unsigned k_hi) {
    const int b = blockIdx.x, tid = threadIdx.x;
    hist[(b * 2) * 256 + tid] = 0;
    hist[(b * 2 + 1) * 256 + tid] = 0;
    if (tid < 2) { st[b].prefix[tid] = 0; st[b].rank[tid] = tid ? k_hi : k_lo; }
}

// grid (chunks of the largest block, blocks, B): digit `pass` (most significant first) of the keys that share the prefix of
// rank 0 / rank 1, counted in LDS and added to hist (B, 2, 256) with integer atomics.
__global__ __launch_bounds__(256) void k_spec_hist(SpecGeom G, const float* __restrict__ db, int pass, const SpecSel* __restrict__ st,
                                                    unsigned* __restrict__ hist) {
    const int k = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
    const int64_t len = (int64_t)G.F[k] * G.N[k], i0 = (int64_t)blockIdx.x * SPEC_HIST_CHUNK;
    if (i0 >= len) return;
    int64_t before = 0;
    for (int q = 0; q < k; ++q) before += (int64_t)G.F[q] * G.N[q];
    const float* v = db + (int64_t)G.B * before + (int64_t)b * len;
    const int shift = 24 - 8 * pass;
    const unsigned mask = pass ? 0xffffffffu << (shift + 8) : 0u;
    const unsigned pre0 = st[b].prefix[0] & mask, pre1 = st[b].prefix[1] & mask;
    const bool same = pre0 == pre1;                 // adjacent ranks mostly share their prefix: one count serves both
    __shared__ unsigned h[2][256];
    h[0][tid] = 0;
    h[1][tid] = 0;
    __syncthreads();
    const int64_t i1 = i0 + SPEC_HIST_CHUNK < len ? i0 + SPEC_HIST_CHUNK : len;
    // neighbouring columns share their leading digits: a thread counts a run in a register and adds it once
    unsigned d0 = 0, n0 = 0, d1 = 0, n1 = 0;
    for (int64_t i = i0 + tid; i < i1; i += 256) {
        const unsigned key = spec_key(v[i]), d = (key >> shift) & 255u;
        if ((key & mask) == pre0) {
            if (d != d0 && n0) { atomicAdd(&h[0][d0], n0); n0 = 0; }
            d0 = d;
            ++n0;
        }
        if (!same && (key & mask) == pre1) {
            if (d != d1 && n1) { atomicAdd(&h[1][d1], n1); n1 = 0; }
            d1 = d;
            ++n1;
        }
    }
    if (n0) atomicAdd(&h[0][d0], n0);
    if (n1) atomicAdd(&h[1][d1], n1);
    __syncthreads();
    const unsigned c0 = h[0][tid], c1 = same ? c0 : h[1][tid];
    if (c0) atomicAdd(&hist[(b * 2) * 256 + tid], c0);
    if (c1) atomicAdd(&hist[(b * 2 + 1) * 256 + tid], c1);
}

// grid (B): the digit that holds each rank, the rank inside it; clears the histogram for the next pass; after the last pass
// the prefix is the key: out (B, 2).
__global__ __launch_bounds__(256) void k_spec_pick(int pass, SpecSel* __restrict__ st, unsigned* __restrict__ hist, float* __restrict__ out) {
    const int b = blockIdx.x, tid = threadIdx.x;
    __shared__ unsigned sc[2][256];
    const unsigned rank0 = st[b].rank[0], rank1 = st[b].rank[1], pre0 = st[b].prefix[0], pre1 = st[b].prefix[1];
    sc[0][tid] = hist[(b * 2) * 256 + tid];
    sc[1][tid] = hist[(b * 2 + 1) * 256 + tid];
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {          // inclusive prefix sums of the 256 counts, both ranks at once
        const unsigned a0 = tid >= off ? sc[0][tid - off] : 0u, a1 = tid >= off ? sc[1][tid - off] : 0u;
        __syncthreads();
        sc[0][tid] += a0;
        sc[1][tid] += a1;
        __syncthreads();
    }
#pragma unroll
    for (int w = 0; w < 2; ++w) {                       // the one digit whose counts straddle the rank
        const unsigned rank = w ? rank1 : rank0, below = tid ? sc[w][tid - 1] : 0u;
        if (below <= rank && rank < sc[w][tid]) {
            const unsigned prefix = (w ? pre1 : pre0) | (unsigned)tid << (24 - 8 * pass);
            st[b].prefix[w] = prefix;
            st[b].rank[w] = rank - below;
            if (pass == 3) out[b * 2 + w] = spec_unkey(prefix);
        }
    }
    hist[(b * 2) * 256 + tid] = 0;
    hist[(b * 2 + 1) * 256 + tid] = 0;
}

// grid (pixel groups, bands, B).  g = lanes per pixel, a power of two near the block's columns per pixel, so that a wave reads
// a contiguous run of the row whatever the pooling factor; SPEC_RASTER_REP groups of 256 / g pixels per workgroup.
__global__ __launch_bounds__(256) void k_spec_raster(SpecGeom G, const float* __restrict__ db, int W, float* __restrict__ img) {
    const SpecAt at = spec_locate(G, blockIdx.y);
    const int F = G.F[at.k], N = G.N[at.k], b = blockIdx.z, tid = threadIdx.x;
    int g = 1;
    while (g < 64 && (int64_t)g * W < N) g <<= 1;
    const int per = 256 / g;
    if ((int64_t)blockIdx.x * per * SPEC_RASTER_REP >= W) return;
    const int sub = tid & (g - 1);
    const float* row = db + (int64_t)G.B * at.out + ((int64_t)b * F + at.f) * N;
    for (int rep = 0; rep < SPEC_RASTER_REP; ++rep) {
        const int w = (blockIdx.x * SPEC_RASTER_REP + rep) * per + tid / g;
        float m = -__builtin_inff();
        if (w < W) {
            const int64_t lo = (int64_t)w * N / W, hi2 = ((int64_t)w + 1) * N / W, hi = hi2 > lo + 1 ? hi2 : lo + 1;
            for (int64_t c = lo + sub; c < hi; c += g) m = fmaxf(m, row[c]);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1)
            if (off < g) m = fmaxf(m, __shfl_xor(m, off, 64));
        if (w < W && sub == 0) img[((int64_t)b * gridDim.y + blockIdx.y) * W + w] = m;
    }
}

static int spec_geom(const char* who, int nblocks, const int32_t* F, const int32_t* T, const int32_t* N, int B, int S, SpecGeom* g,
                     int64_t* bands, int64_t* longest_row, int64_t* largest_block, int64_t* total) {
    XSQ_REQUIRE(nblocks > 0 && F && T, "%s: null block table", who);
    XSQ_REQUIRE(nblocks <= SPEC_MAX_BLOCKS, "%s: %d blocks; the geometry goes to the kernels by value and holds %d", who, nblocks, SPEC_MAX_BLOCKS);
    XSQ_REQUIRE(B > 0 && B <= 65535 && S >= 1, "%s: B=%d S=%d (1 <= B <= 65535, S >= 1)", who, B, S);
    g->nblocks = nblocks; g->B = B; g->S = S;
    *bands = *longest_row = *largest_block = *total = 0;
    for (int k = 0; k < nblocks; ++k) {
        XSQ_REQUIRE(F[k] > 0 && T[k] > 0 && T[k] % 4 == 0, "%s: block %d has F=%d T=%d (T a positive multiple of 4)", who, k, F[k], T[k]);
        XSQ_REQUIRE((int64_t)S * T[k] < 0x7fffffff, "%s: block %d: S * T = %lld columns exceed 2^31", who, k, (long long)S * T[k]);
        g->F[k] = F[k]; g->T[k] = T[k]; g->N[k] = N ? N[k] : 0;
        *bands += F[k];
        if (N) {
            XSQ_REQUIRE(N[k] >= 1, "%s: block %d has N=%d columns (the signal is too short for this block)", who, k, N[k]);
            *longest_row = N[k] > *longest_row ? N[k] : *longest_row;
            const int64_t blk = (int64_t)F[k] * N[k];
            *largest_block = blk > *largest_block ? blk : *largest_block;
            *total += blk;
        }
    }
    XSQ_REQUIRE(*bands <= 65535, "%s: %lld bands exceed one launch", who, (long long)*bands);
    return XSQ_OK;
}

// N against what the slices hold: (S - 1) h columns after the crop, S T - T when flattened
static int spec_columns_ok(const char* who, const SpecGeom& g, int flatten) {
    for (int k = 0; k < g.nblocks; ++k) {
        const int64_t most = flatten ? (int64_t)g.S * g.T[k] - g.T[k] : (int64_t)(g.S - 1) * (g.T[k] / 2);
        XSQ_REQUIRE(g.N[k] <= most, "%s: block %d: N=%d columns, the %d slices of %d hold %lld", who, k, g.N[k], g.S, g.T[k], (long long)most);
    }
    return XSQ_OK;
}

}  // namespace xsq

using namespace xsq;

extern "C" {

int xsq_spectrogram_max_blocks(void) { return SPEC_MAX_BLOCKS; }

int64_t xsq_spectrogram_overlap_add_size(int nblocks, const int32_t* F, const int32_t* T, int BC, int S, int flatten) {
    if (nblocks <= 0 || !F || !T || BC <= 0 || S <= 0) return 0;
    int64_t n = 0;
    for (int k = 0; k < nblocks; ++k) n += 2 * (int64_t)BC * F[k] * (flatten ? (int64_t)S * T[k] : (int64_t)(S + 1) * (T[k] / 2));
    return n;
}

int xsq_spectrogram_overlap_add(int nblocks, const int32_t* F, const int32_t* T, const float* arena, int BC, int S, int flatten, float* out,
                                void* stream_) {
    const char* who = "xsq_spectrogram_overlap_add";
    XSQ_REQUIRE(arena && out, "%s: null argument", who);
    XSQ_REQUIRE(((uintptr_t)arena & 15) == 0 && ((uintptr_t)out & 15) == 0, "%s: arena and out must be 16-byte aligned", who);
    SpecGeom g;
    int64_t bands, a, b, c;
    if (int rc = spec_geom(who, nblocks, F, T, nullptr, BC, S, &g, &bands, &a, &b, &c)) return rc;
    int64_t longest = 0;
    for (int k = 0; k < nblocks; ++k) {
        const int64_t L = flatten ? (int64_t)S * T[k] : (int64_t)(S + 1) * (T[k] / 2);
        longest = L > longest ? L : longest;
    }
    const dim3 grid((unsigned)((longest + SPEC_CHUNK - 1) / SPEC_CHUNK), (unsigned)bands, (unsigned)BC);
    hipStream_t stream = (hipStream_t)stream_;
    { XSQ_PROF("spec_ola", stream);
      if (flatten) hipLaunchKernelGGL(k_spec_ola<true>, grid, dim3(256), 0, stream, g, arena, out);
      else hipLaunchKernelGGL(k_spec_ola<false>, grid, dim3(256), 0, stream, g, arena, out); }
    XSQ_HIP(hipGetLastError());
    return XSQ_OK;
}

int xsq_spectrogram_db(int nblocks, const int32_t* F, const int32_t* T, const int32_t* N, const float* arena, int B, int S, int flatten,
                       float* db, void* stream_) {
    const char* who = "xsq_spectrogram_db";
    XSQ_REQUIRE(arena && db && N, "%s: null argument", who);
    XSQ_REQUIRE(((uintptr_t)arena & 15) == 0, "%s: the arena must be 16-byte aligned", who);
    SpecGeom g;
    int64_t bands, longest, largest, total;
    if (int rc = spec_geom(who, nblocks, F, T, N, B, S, &g, &bands, &longest, &largest, &total)) return rc;
    XSQ_REQUIRE(S >= 2, "%s: S=%d; the crop leaves nothing of fewer than two slices", who, S);
    if (int rc = spec_columns_ok(who, g, flatten)) return rc;
    const dim3 grid((unsigned)((longest + SPEC_CHUNK - 1) / SPEC_CHUNK), (unsigned)bands, (unsigned)B);
    hipStream_t stream = (hipStream_t)stream_;
    { XSQ_PROF("spec_db", stream);
      if (flatten) hipLaunchKernelGGL(k_spec_db<true>, grid, dim3(256), 0, stream, g, arena, db);
      else hipLaunchKernelGGL(k_spec_db<false>, grid, dim3(256), 0, stream, g, arena, db); }
    XSQ_HIP(hipGetLastError());
    return XSQ_OK;
}

size_t xsq_spectrogram_order_workspace(int B) { return B > 0 ? al256((size_t)B * (2 * 256 * 4 + sizeof(SpecSel))) : 0; }

int xsq_spectrogram_order_stats(int nblocks, const int32_t* F, const int32_t* N, const float* db, int B, int64_t k_lo, int64_t k_hi,
                                float* out, void* ws, size_t ws_bytes, void* stream_) {
    const char* who = "xsq_spectrogram_order_stats";
    XSQ_REQUIRE(db && out && ws && N, "%s: null argument", who);
    SpecGeom g;
    int64_t bands, longest, largest, total;
    int32_t T4[SPEC_MAX_BLOCKS];
    for (int k = 0; k < SPEC_MAX_BLOCKS; ++k) T4[k] = 4;                   // the select does not look at T
    if (int rc = spec_geom(who, nblocks, F, T4, N, B, 2, &g, &bands, &longest, &largest, &total)) return rc;
    XSQ_REQUIRE(total < 0xffffffffll, "%s: %lld values per batch item; the counts are 32-bit", who, (long long)total);
    XSQ_REQUIRE(0 <= k_lo && k_lo <= k_hi && k_hi <= k_lo + 1 && k_hi < total, "%s: ranks %lld, %lld of %lld values", who, (long long)k_lo,
                (long long)k_hi, (long long)total);
    XSQ_REQUIRE(ws_bytes >= xsq_spectrogram_order_workspace(B), "%s: workspace too small (%zu needed, %zu given)", who,
                xsq_spectrogram_order_workspace(B), ws_bytes);
    unsigned* hist = (unsigned*)ws;
    SpecSel* st = (SpecSel*)(hist + (size_t)B * 2 * 256);
    hipStream_t stream = (hipStream_t)stream_;
    const dim3 grid((unsigned)((largest + SPEC_HIST_CHUNK - 1) / SPEC_HIST_CHUNK), (unsigned)nblocks, (unsigned)B);
    hipLaunchKernelGGL(k_spec_sel_init, dim3(B), dim3(256), 0, stream, st, hist, (unsigned)k_lo, (unsigned)k_hi);
    for (int pass = 0; pass < 4; ++pass) {
        { XSQ_PROF("spec_hist", stream);
          hipLaunchKernelGGL(k_spec_hist, grid, dim3(256), 0, stream, g, db, pass, (const SpecSel*)st, hist); }
        { XSQ_PROF("spec_pick", stream);
          hipLaunchKernelGGL(k_spec_pick, dim3(B), dim3(256), 0, stream, pass, st, hist, out); }
    }
    XSQ_HIP(hipGetLastError());
    return XSQ_OK;
}

int xsq_spectrogram_raster(int nblocks, const int32_t* F, const int32_t* N, const float* db, int B, int W, float* image, void* stream_) {
    const char* who = "xsq_spectrogram_raster";
    XSQ_REQUIRE(db && image && N, "%s: null argument", who);
    XSQ_REQUIRE(W >= 1 && W <= (1 << 24), "%s: width %d (1 .. 2^24)", who, W);
    SpecGeom g;
    int64_t bands, longest, largest, total;
    int32_t T4[SPEC_MAX_BLOCKS];
    for (int k = 0; k < SPEC_MAX_BLOCKS; ++k) T4[k] = 4;                   // the raster does not look at T
    if (int rc = spec_geom(who, nblocks, F, T4, N, B, 2, &g, &bands, &longest, &largest, &total)) return rc;
    // the block with the fewest columns per pixel has the most pixels per workgroup; the grid covers the one with the fewest
    int gmax = 1;
    while (gmax < 64 && (int64_t)gmax * W < longest) gmax <<= 1;
    const int per = 256 / gmax;
    hipStream_t stream = (hipStream_t)stream_;
    { XSQ_PROF("spec_raster", stream);
      hipLaunchKernelGGL(k_spec_raster, dim3((unsigned)((W + per * SPEC_RASTER_REP - 1) / (per * SPEC_RASTER_REP)), (unsigned)bands, (unsigned)B), dim3(256), 0, stream, g, db, W, image); }
    XSQ_HIP(hipGetLastError());
    return XSQ_OK;
}

}  // extern "C"
