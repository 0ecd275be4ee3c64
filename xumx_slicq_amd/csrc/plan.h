// Host-side plan object behind the C ABI (include/xumx_slicq_hip.h).
#pragma once
#include <algorithm>
#include <map>
#include <mutex>
#include <tuple>
#include <vector>

#include <rocfft/rocfft.h>

#include "common.h"

namespace xsq {

struct FftPlan {
    rocfft_plan plan = nullptr;
    rocfft_execution_info info = nullptr;
    size_t work_bytes = 0;
};

struct TileTable {
    TileDev* d_tiles = nullptr;     // (entries of the builder's own type: cast at the launch sites)
    int ntiles = 0;
};

// Key of a cached tile table: the builder, the call shape and the builder's own parameters, each in a field of its own --
// two builders, or two parameter sets of one builder, cannot meet in one key.
enum class TileKind { BandGemm, Dft4Full, CdaeGemm, CdaeSlab, CdaeWino, CdaeWino23, CdaeL1f, CdaeL4f };
struct TileKey {
    TileKind kind;
    int rows, S;        // call shape: rows of the transform (S = `share`) / batch items and slices of the CDAE
    int sub, flags;     // which table of the builder (CDAE layer) / its switches, named at the builder
    bool operator<(const TileKey& o) const {
        return std::tie(kind, rows, S, sub, flags) < std::tie(o.kind, o.rows, o.S, o.sub, o.flags);
    }
};

// `count` elements at src -> a fresh device allocation at dst.  No elements: dst stays null and the call succeeds; a failed copy
// frees what it allocated and leaves dst null.  (dst may be declared with another element type than T, or as void*.)
template <class D, class T>
static int upload(D*& dst, const T* src, size_t count) {
    dst = nullptr;
    if (!count) return XSQ_OK;
    XSQ_HIP(hipMalloc((void**)&dst, count * sizeof(T)));
    const hipError_t e = hipMemcpy(dst, src, count * sizeof(T), hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(dst); dst = nullptr; }
    XSQ_HIP(e);
    return XSQ_OK;
}
template <class D, class T>
static int upload(D*& dst, const std::vector<T>& vec) { return upload(dst, vec.data(), vec.size()); }

// The table of `key` from the owner's cache, or built by fill(std::vector<T>&), uploaded and inserted.  An empty table has no
// allocation (d_tiles null, ntiles 0).
template <class T, class Fill>
static int cached_tiles(std::mutex& mu, std::map<TileKey, TileTable>& cache, const TileKey& key, TileTable* out, Fill&& fill) {
    std::lock_guard<std::mutex> lk(mu);
    auto it = cache.find(key);
    if (it != cache.end()) { *out = it->second; return XSQ_OK; }
    std::vector<T> t;
    fill(t);
    TileTable tt;
    tt.ntiles = (int)t.size();
    if (int rc = upload(tt.d_tiles, t)) return rc;
    cache[key] = tt;
    *out = tt;
    return XSQ_OK;
}

// the indices 0 .. n - 1 ordered by key(i), descending, stable (longest tiles first: a launch ends on short tiles)
template <class KeyFn>
static std::vector<int> order_descending(int n, KeyFn key) {
    std::vector<int> order(n);
    for (int i = 0; i < n; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return key(x) > key(y); });
    return order;
}

struct BlockHost {
    int first_band, F, T;
    int64_t cum;  // sum of F*T over earlier blocks
};

}  // namespace xsq

struct xsq_plan {
    int L = 0, tr = 0, h = 0, nbins = 0, nbands = 0, nblocks = 0;
    int64_t sumFT = 0;  // complex coefficients per channel-slice (18640 for Bark-262)
    std::vector<xsq::BandDev> bands;
    std::vector<xsq::BlockHost> blocks;
    // device tables
    int band_radix4 = 1;            // 1: bands with Lg >= 24 (XSQ_D4_MIN_LG_DEFAULT) run on the radix-4 kernel (band_dft4.h), 0: all on the dense GEMM
    void* d_bands4 = nullptr;       // Band4Dev table of the eligible bands
    float* d_pool4f = nullptr;      // DFT_m matrices, twiddles, windows: analysis direction
    float* d_pool4i = nullptr;      //                                     synthesis direction
    int nbands4 = 0;
    std::vector<unsigned char> bands4_host;    // host copy of the Band4Dev table (the tile entries carry their band's descriptor)
    int64_t d4_max_block = 0;                  // largest F * Lg of a radix-4 band's arena block (buffer ranges of band_dft4.h)
    std::vector<int> bands4_m, bands4_small;   // host copies: m of each eligible band; indices of the other bands
    int fft_backend = 0;            // 0: hand-written LDS FFT when L == 18060, else rocFFT; 1: always rocFFT
    float2* d_T = nullptr;          // twiddles of the hand-written slice FFT: w1 (43*210) | w2 (14*15) | wl (L/2+1)
    unsigned short* d_tgt16 = nullptr;   // the same table as 16-bit bins (0xFFFF = none) + one pad entry: pairs of entries load as one dword
    int* d_tgt = nullptr;           // (sumFT) target bin per phase-ordered entry; null if bands of one phase overlap
    int phase_begin[5] = {0, 0, 0, 0, 0};
    // short bands (below the radix-4 split) synthesised inside k_slice_irfft (slice_fft.h: ShortSched); valid when short_n1 > 0
    int packed_fft = 0;             // 1: slice FFT codelets on v_pk_* (xsq_plan_set_packed_fft; only beside fp32 contractions)
    int short_inline = 0;           // 0 (default, faster as measured): short bands on the dense GEMM + Z round trip (band_synthesis_gemm)
    void *d_s_item1 = nullptr, *d_s_tw1 = nullptr;
    int *d_s_item2 = nullptr, *d_s_tgt = nullptr;
    float* d_s_wd = nullptr;
    int short_n1 = 0, short_n2 = 0, short_nent = 0, short_sc0 = 0;
    int short_begin[5] = {0, 0, 0, 0, 0};
    int phase_long[4] = {0, 0, 0, 0};   // first entry of each gather phase that belongs to a band NOT handled in-kernel
    float* d_tw = nullptr;          // (L) slice window
    float* d_Wf = nullptr;          // per-band analysis matrices  (window, sign, 1/Lg folded in)
    float* d_Wi = nullptr;          // per-band synthesis matrices (dual window, Lg, sign, 1/L folded in)
    xsq::BandDev* d_bands = nullptr;
    int* d_cov_ptr = nullptr;       // (nbins+1) CSR over spectrum bins -> covering bands
    int* d_cov_band = nullptr;
    // Adjoint of the inverse transform (xsq_slicqt_inverse_adjoint): the analysis tables rebuilt from the adjoint window a'
    // (xsq_slicqt_adjoint_window) and a slice window of ones, on first use, from the host copies of the band table kept here.
    std::vector<int32_t> h_Lg, h_c;
    std::vector<double> h_gd;
    size_t wf_floats = 0, pool4_floats = 0;   // sizes of d_Wf and d_pool4f as built: the adjoint's copies must have the same layout
    bool adj_built = false;
    float* d_adj_tw = nullptr;      // (L) ones
    float* d_adj_Wf = nullptr;      // dense analysis matrices of a'
    float* d_adj_pool4f = nullptr;  // radix-4 analysis pool with the windows a'
    // Adjoint of the forward transform (xsq_slicqt_forward_adjoint): the synthesis tables rebuilt from the window
    // xsq_slicqt_forward_adjoint_window makes of g, and the fold list (slicqt.hip: FoldDst / FoldSrc), on first use.
    std::vector<float> h_g;
    bool fadj_built = false;
    float* d_fadj_Wi = nullptr;     // dense synthesis matrices of that window
    float* d_fadj_pool4i = nullptr; // radix-4 synthesis pool with it
    void *d_fold_dst = nullptr, *d_fold_src = nullptr;            // the rocFFT path's: a pass over Z (k_fold_mirrored)
    int nfold_dst = 0;
    void *d_fold_inl_dst = nullptr, *d_fold_inl_src = nullptr;    // the hand-written slice FFT's: inside k_slice_irfft (FoldSched)
    int nfold_inl = 0;
    // The mirrored synthesis of the bands that reach across DC (dc_twins.h): made by xsq_plan_create_twins alone, so a plan of
    // xsq_plan_create has ntwins == 0 and launches nothing for it.  Such a plan always takes the rocFFT path (lds_fft).
    void *d_twin_bins = nullptr, *d_twin_src = nullptr;     // synthesis: TwinDst per landing bin / TwinSrc per entry
    void *d_twin_bands = nullptr, *d_twin_asrc = nullptr;   // its transpose: TwinDst per band / TwinSrc per entry
    float2* d_twin_tw = nullptr;                            // e^{2 pi i r / Lg}, r = 0 .. Lg - 1, per distinct Lg of those bands
    int ntwin_bins = 0, ntwin_bands = 0, ntwins = 0;        // ntwins: landing entries (xsq_plan_num_twins)
    // The FFT band engine (band_fft.h): on a plan of xsq_plan_create_flags with XSQ_PLAN_LONG_BANDS every band above LONG_LG runs there
    // and has no dense matrix; any other plan has nlong == 0 and launches nothing for it.  Such a plan with a long band takes the
    // rocFFT path (lds_fft).
    bool long_bands = false;
    std::vector<char> on_fft;                       // (nbands) 1: the band runs on the FFT band engine
    void* d_long = nullptr;                         // LongBandDev table, classes of equal N back to back, largest N first
    int nlong = 0;
    std::vector<std::tuple<int, int, int>> long_classes;   // (first entry, entries, N)
    float *d_poolLf = nullptr, *d_poolLi = nullptr; // chirps, transformed chirps, twiddles, windows: analysis / synthesis direction
    size_t poolL_floats = 0;
    float *d_adj_poolLf = nullptr, *d_fadj_poolLi = nullptr;   // the same pools over the adjoints' windows
    // caches keyed by the call shape
    std::mutex mu;
    std::map<std::pair<int, int>, xsq::FftPlan> fft;              // (direction, batch)
    std::map<xsq::TileKey, xsq::TileTable> tiles;
};
