// One training batch from the device-resident stem pool in one launch, gfx950.
//
// Reference: xumx_slicq_v2/data.py:316-390 (MUSDBDataset.__getitem__ with random_track_mix) and the DataLoader's collate:
// per item and source a track is picked, an excerpt of seq_duration is cut, `audio * g` (data.py:188) and a channel flip
// (data.py:191-196) are applied, the four excerpts are stacked and summed into the mix (data.py:362-364), and B items are
// stacked into a batch.  Here the stems of every track stay on the device (fp32, or the files' 16-bit PCM), the host draws an
// epoch's (track, start, gain, swap) records once, and k_batch_assemble turns one step's records into x (B, 2, n) and
// y (4, B, 2, n): every output element is read from the pool, scaled, summed and written once.
//
// Arithmetic (held bitwise by tests/test_data_gpu.py): v = pool sample (pcm16: float(int) * 2^-15, exact), 0 past the track's
// end; y = fl32(gain * v); x = ((y_0 + y_1) + y_2) + y_3 in source-column order.  No contraction: the product is rounded before
// the sums, as torch's `audio * g` followed by `stems.sum(0)` rounds it.
//
// One thread owns four consecutive samples of one (b, c) row of x, aligned to that row's 16-byte boundaries, and the same four
// samples of the four target rows.  The four source rows start at arbitrary offsets: a row whose four samples sit on a
// 4-element boundary is read with one wide load (16 bytes fp32, 8 bytes pcm16), any other with the two aligned windows that
// cover them, and only the ends of a row -- the lead-in in front of the first boundary, the last samples before `len` -- element
// by element.  Nothing is read at or past a row's `len`.  A target row that shares x's alignment (all of them when n is even)
// is stored 16 bytes at a time; with odd n the rows of every other target plane are two floats off and take 4-byte stores.
#include "../../include/xumx_slicq_hip.h"
#include "common.h"
#include "prof.h"

namespace xsq {

constexpr int BATCH_THREADS = 256;

struct BatchArgs {
    const void* pool;
    const int64_t* tracks;        // ntracks x (element offset of row (0, 0), length in samples)
    const int32_t* draws;         // this step's records: [B][4][track, start, gain bits, swap]
    const int32_t* target_of_column;
    float* x;
    float* y;
    int64_t n;
    int B, ntracks;
};

__device__ __forceinline__ float pool_value(float v) { return v; }
__device__ __forceinline__ float pool_value(short v) { return (float)(int)v * 0x1p-15f; }

template <class T> struct Vec4;
template <> struct Vec4<float> { typedef float4 type; };
template <> struct Vec4<short> { typedef short4 type; };

// samples [p, p + 4) of a row of `len` samples into o[]; 0 outside [0, len)
template <class T>
__device__ __forceinline__ void load4(const T* __restrict__ row, int64_t p, int64_t len, float o[4]) {
    typedef typename Vec4<T>::type V;
    const int sh = (int)((reinterpret_cast<uintptr_t>(row + p) / sizeof(T)) & 3);   // elements behind the last 4-element boundary
    const int64_t q = p - sh;
    if (sh == 0 && p >= 0 && p + 4 <= len) {
        const V a = *reinterpret_cast<const V*>(row + p);
        o[0] = pool_value(a.x); o[1] = pool_value(a.y); o[2] = pool_value(a.z); o[3] = pool_value(a.w);
    } else if (sh != 0 && q >= 0 && q + 8 <= len) {
        const V a = *reinterpret_cast<const V*>(row + q), b = *reinterpret_cast<const V*>(row + q + 4);
        const float w1 = pool_value(a.y), w2 = pool_value(a.z), w3 = pool_value(a.w);
        const float w4 = pool_value(b.x), w5 = pool_value(b.y), w6 = pool_value(b.z);
        o[0] = sh == 1 ? w1 : sh == 2 ? w2 : w3;
        o[1] = sh == 1 ? w2 : sh == 2 ? w3 : w4;
        o[2] = sh == 1 ? w3 : sh == 2 ? w4 : w5;
        o[3] = sh == 1 ? w4 : sh == 2 ? w5 : w6;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (p + j >= 0 && p + j < len) ? pool_value(row[p + j]) : 0.f;
    }
}

__device__ __forceinline__ void store4(float* __restrict__ d, int64_t u, int64_t n, const float v[4]) {
    if (u >= 0 && u + 4 <= n && (reinterpret_cast<uintptr_t>(d + u) & 15) == 0) {
        *reinterpret_cast<float4*>(d + u) = make_float4(v[0], v[1], v[2], v[3]);
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (u + j >= 0 && u + j < n) d[u + j] = v[j];
}

template <class T>
__global__ __launch_bounds__(BATCH_THREADS) void k_batch_assemble(const BatchArgs A) {
#pragma clang fp contract(off)
    const int bc = blockIdx.y, b = bc >> 1, c = bc & 1;
    float* xr = A.x + (int64_t)bc * A.n;
    const int lead = (int)((reinterpret_cast<uintptr_t>(xr) >> 2) & 3);     // floats of the row behind the last 16-byte boundary
    const int64_t u = ((int64_t)blockIdx.x * BATCH_THREADS + threadIdx.x) * 4 - lead;
    if (u >= A.n) return;
    const T* pool = static_cast<const T*>(A.pool);
    float mix[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int32_t* rec = A.draws + ((int64_t)b * 4 + s) * 4;
        const int t = min(max(rec[0], 0), A.ntracks - 1);
        const int64_t start = rec[1];
        const float gain = __int_as_float(rec[2]);
        const int cs = c ^ (rec[3] & 1);
        const int64_t off = A.tracks[2 * t], len = A.tracks[2 * t + 1];
        const int64_t stride = (len + 7) & ~(int64_t)7;
        float v[4];
        load4(pool + off + (int64_t)(2 * s + cs) * stride, start + u, len, v);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[j] = __fmul_rn(gain, v[j]);
            mix[j] = s == 0 ? v[j] : __fadd_rn(mix[j], v[j]);
        }
        const int plane = A.target_of_column[s] & 3;
        store4(A.y + (((int64_t)plane * A.B + b) * 2 + c) * A.n, u, A.n, v);
    }
    store4(xr, u, A.n, mix);
}

}  // namespace xsq

using namespace xsq;

extern "C" int xsq_batch_assemble(const void* pool, int pool_dtype, const int64_t* tracks, int ntracks, const int32_t* draws,
                                  int64_t step, int B, int64_t n, const int32_t* target_of_column, float* x, float* y,
                                  void* stream) {
    XSQ_REQUIRE(pool && tracks && draws && target_of_column && x && y, "xsq_batch_assemble: null pointer");
    XSQ_REQUIRE(pool_dtype == XSQ_POOL_FP32 || pool_dtype == XSQ_POOL_PCM16, "xsq_batch_assemble: pool dtype %d (0: fp32, 1: pcm16)",
                pool_dtype);
    XSQ_REQUIRE(B >= 1 && B <= 32767 && n >= 1 && n < (1ll << 31) && ntracks >= 1 && step >= 0,
                "xsq_batch_assemble: B=%d (1 .. 32767) n=%lld (1 .. 2^31 - 1) ntracks=%d step=%lld", B, (long long)n, ntracks,
                (long long)step);
    XSQ_REQUIRE((reinterpret_cast<uintptr_t>(pool) & 15) == 0 && (reinterpret_cast<uintptr_t>(x) & 3) == 0 &&
                    (reinterpret_cast<uintptr_t>(y) & 3) == 0,
                "xsq_batch_assemble: the pool must be 16-byte aligned, x and y 4-byte aligned");
    BatchArgs A;
    A.pool = pool; A.tracks = tracks; A.draws = draws + step * (int64_t)B * 16; A.target_of_column = target_of_column;
    A.x = x; A.y = y; A.n = n; A.B = B; A.ntracks = ntracks;
    hipStream_t st = (hipStream_t)stream;
    const int64_t gx = (n + 3 + 4 * BATCH_THREADS - 1) / (4 * BATCH_THREADS);          // + 3: the row's lead-in
    const dim3 grid((unsigned)gx, (unsigned)(2 * B));
    XSQ_PROF("batch_assemble", st);
    if (pool_dtype == XSQ_POOL_PCM16)
        hipLaunchKernelGGL(k_batch_assemble<short>, grid, dim3(BATCH_THREADS), 0, st, A);
    else
        hipLaunchKernelGGL(k_batch_assemble<float>, grid, dim3(BATCH_THREADS), 0, st, A);
    XSQ_HIP(hipGetLastError());
    return XSQ_OK;
}
