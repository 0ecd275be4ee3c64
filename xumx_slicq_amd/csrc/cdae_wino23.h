// Layers 2 and 3 of the CDAE (fp32) in ONE launch for the blocks with a single frequency tap (kf == 1): both as Winograd
// F(2, 4) along the time taps (cdae_wino.h), layer 2's output handed to layer 3 in LDS.
//
// With one frequency tap, row f of act3 needs row f of act2 needs row f of act1 (F1 == F2), and a tile of cdae_wino_kernel is
// three chunks of issue work between a prologue that waits for HBM and an epilogue of cross-lane sums and stores.  Here a tile
// runs both layers: one prologue, six chunks, one epilogue, and act2 of these blocks never goes to HBM.
//
// Tile = 62 consecutive act3 pairs [A, A + 62) of ONE (b, f) row.  act3 pair q reads act2 positions 2 q - 3 .. 2 q + 1, i.e.
// act2 pairs q - 2 .. q: the tile's 64 lanes first compute act2 pairs A - 2 .. A + 61 (stage 1 = the body of
// cdae_wino_kernel<false> on the act1 slab of positions 2 (A - 2) .. 2 (A - 2) + 130), write them over the slab planes in the
// layout stage 2 reads (local position j' = act2 position - (2 A - 3): plane j' & 1, row j' >> 1 -- output 0 of lane p lands in
// odd row p - 1, output 1 in even row p), and after one barrier run the body of cdae_wino_kernel<true> on them (lanes 62 and 63
// compute pairs nobody stores).  act2 positions outside [0, T2) are written as zeros: the transposed convolution's padding,
// what the buffer loads of the two-launch form return out of range.
//
// Every value goes through the operations of the two kernels in their order (fp contract off, FMAs spelled out; a pair's
// accumulators depend on its own MFMA column only), so act3 is what the two launches produce, bit for bit
// (tests/test_cdae_fused23_gpu.py).  The weight stream runs through both stages on one chunk counter and the two LDS buffers:
// layer 3's first chunk is requested during layer 2's last.  LDS and launch bounds are those of cdae_wino_kernel.
#pragma once
#include "cdae_wino.h"

namespace xsq {

constexpr int WN23_OUT = WN_PAIRS - 2;                    // act3 pairs per fused tile (62)

struct Wino23TileDev {             // 64 bytes: one scalar load
    int A, f, F, b;                // first act3 pair of the tile in its row, the row, rows of the (block, target), batch item
    int64_t in_off, out_off;       // act1 / act3 of the (block, target), relative to the arenas
    int64_t shift2_off, shift3_off;    // shift vectors inside the pool
    int64_t u2_off, u3_off;        // transformed weights inside the Winograd pool
};
static_assert(sizeof(Wino23TileDev) == 64, "Wino23TileDev is meant to be one 64-byte scalar load");

template <int NV> struct Wino23Frag { float4 w[3]; float u[NV]; float wt[3]; float ut[NV]; };

__global__ __launch_bounds__(256, XSQ_WINO_WAVES_PER_EU) void cdae_wino23_kernel(CdaeArgs a, const Wino23TileDev* __restrict__ tiles, int ntiles) {
#pragma clang fp contract(off)
    constexpr int PLANE_O = WN_EROWS * WN_SLD;                   // word offset of the odd plane
    __shared__ __attribute__((aligned(16))) float slab[(WN_EROWS + WN_OROWS) * WN_SLD];
    __shared__ __attribute__((aligned(16))) float Bs[2 * 5 * WN_BTILE];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = lane & 15, kq = lane >> 4;
    const Wino23TileDev t = tiles[xcd_remap(blockIdx.x, ntiles)];
    asm volatile("" :: "s"(t.A), "s"(t.f), "s"(t.F), "s"(t.b), "s"(t.in_off), "s"(t.out_off), "s"(t.shift2_off), "s"(t.shift3_off),
                 "s"(t.u2_off), "s"(t.u3_off));
    const int A = t.A, f = t.f, F = t.F, b = t.b;
    const int T1 = a.T1, T2 = a.T2;

    // ---- weight stream (cdae_wino.h): chunk s of a layer = five component tiles of 51 columns -> the LDS buffer the chunk counter picks
    const __amdgpu_buffer_rsrc_t ru2 = buf_rsrc(a.upool + t.u2_off, 4u * (unsigned)WN_UDF);
    const __amdgpu_buffer_rsrc_t ru3 = buf_rsrc(a.upool + t.u3_off, 4u * (unsigned)WN_UDF);
    const int b_lds0 = (tid >> 2) * WN_BLD + 4 * (tid & 3);
    float4 gb[5];
    auto load_chunk = [&](const __amdgpu_buffer_rsrc_t& ru, int s) {
        const int so = 4 * (s * WN_U16);
#pragma unroll
        for (int r = 0; r < 4; ++r) gb[r] = buf_ld4(ru, (r < 3 || tid < WN_U16 / 4 - 768) ? 16u * (unsigned)(tid + 256 * r) : BUF_OOB, so);
        if (s == 2) gb[4] = buf_ld4(ru, tid < WN_UT / 4 ? 16u * (unsigned)tid : BUF_OOB, 4 * (3 * WN_U16));
    };
    auto store_chunk = [&](int s, int buf) {
        float* Bw = Bs + buf * 5 * WN_BTILE;
#pragma unroll
        for (int r = 0; r < 4; ++r)
            *reinterpret_cast<float4*>(&Bw[(r < 3 || tid < WN_U16 / 4 - 768) ? b_lds0 + 64 * r * WN_BLD : (tid - (WN_U16 / 4 - 768)) * WN_BLD + 20]) = gb[r];
        if (s == 2) *reinterpret_cast<float4*>(&Bw[tid < WN_UT / 4 ? tid * WN_BLD + 16 : 20]) = gb[4];
    };

    // ---- prologue: layer 2's chunk 0 requested, then the act1 slab (cdae_wino.h, one segment): lane = (position lane p0 = tid / 13
    // of 19, channel quad c4 = tid % 13), load r -> local position j = p0 + 19 r = act1 position 2 (A - 2) + j of row f, into plane
    // j & 1, row j >> 1; positions outside the row come back as zeros
    constexpr int SPL = 256 / (CS / 4);                          // position lanes (19)
    constexpr int NPOS = 2 * WN_PAIRS + 3;                       // slab positions of a tile (131)
    constexpr int NLD = (NPOS + SPL - 1) / SPL;                  // loads per lane (7)
    load_chunk(ru2, 0);
    {
        const __amdgpu_buffer_rsrc_t rin = buf_rsrc(a.act1 + t.in_off, 0x40000000u);    // (a (block, target)'s input is < 2^30 bytes: cdae_launch_layer)
        const int s_p0 = tid / (CS / 4), s_c4 = tid - s_p0 * (CS / 4);
        const bool s_on = tid < SPL * (CS / 4);
        float4 sv[NLD];
#pragma unroll
        for (int r = 0; r < NLD; ++r) {
            const int j = s_p0 + SPL * r;
            const int pos = 2 * (A - 2) + j;
            const bool inr = s_on && j < NPOS && (unsigned)pos < (unsigned)T1;
            sv[r] = buf_ld4(rin, inr ? 4u * (unsigned)(((b * F + f) * T1 + pos) * CS + 4 * s_c4) : BUF_OOB, 0);
        }
#pragma unroll
        for (int r = 0; r < NLD; ++r) {
            const int j = s_p0 + SPL * r;
            if (s_on && j < NPOS) *reinterpret_cast<float4*>(&slab[((j & 1) ? PLANE_O : 0) + (j >> 1) * WN_SLD + 4 * s_c4]) = sv[r];
        }
    }
    store_chunk(0, 0);
    __syncthreads();

    const int bf = q * WN_BLD + 4 * kq;                          // weight tile: column q of a 16-column block, k-quad kq
    const int bv = 48 * WN_BLD + 4 * kq + (q & 3);               // the vector columns' weights: one word per lane (cdae_wino.h)
    const int pl = wave * 16 + q;                                // this lane's pair of the tile (act2 pair A - 2 + pl, then act3 pair A + pl)
    const int eb = pl * WN_SLD + 4 * kq;                         // even plane: rows pl, pl + 1, pl + 2 = positions 0, 2, 4 of the pair
    const int ob = PLANE_O + pl * WN_SLD + 4 * kq;               // odd plane: rows pl, pl + 1 = positions 1, 3

    f32x4 acc[5][3];
    float accv[5][3];
    int cnt = 0;                                                 // chunks issued so far: chunk c lives in buffer c & 1

    // one layer's three chunks on the planes (the chunk body of cdae_wino_kernel, weights as the MFMA's row operand); `last`:
    // nothing follows, else layer 3's first chunk is requested during the last chunk
    auto run_layer = [&](auto nv_, auto last_, const __amdgpu_buffer_rsrc_t& ru) {
        constexpr int NV = decltype(nv_)::value;
        constexpr bool last = decltype(last_)::value;
#pragma unroll
        for (int j = 0; j < 5; ++j) {
#pragma unroll
            for (int cb = 0; cb < 3; ++cb) acc[j][cb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int cc = 0; cc < NV; ++cc) accv[j][cc] = 0.f;
        }
        auto read_frag = [&](Wino23Frag<NV>& fr, const float* Bt, bool tail) {
            fr.w[0] = *reinterpret_cast<const float4*>(&Bt[bf]);
            fr.w[1] = *reinterpret_cast<const float4*>(&Bt[bf + 16 * WN_BLD]);
            fr.w[2] = *reinterpret_cast<const float4*>(&Bt[bf + 32 * WN_BLD]);
#pragma unroll
            for (int cc = 0; cc < NV; ++cc) fr.u[cc] = Bt[bv + cc * WN_BLD];
            if (tail) {                                                // channel 48 + kq: word 16 + kq of the row
                const int tb = q * WN_BLD + 16 + kq;
                fr.wt[0] = Bt[tb]; fr.wt[1] = Bt[tb + 16 * WN_BLD]; fr.wt[2] = Bt[tb + 32 * WN_BLD];
#pragma unroll
                for (int cc = 0; cc < NV; ++cc) fr.ut[cc] = Bt[(48 + cc) * WN_BLD + 16 + kq];
            }
        };
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            const int cur = cnt & 1;
            if (s < 2) load_chunk(ru, s + 1);
            else if (!last) load_chunk(ru3, 0);
            const float* Bc = Bs + cur * 5 * WN_BTILE;
            float4 dn[5];
            dn[0] = *reinterpret_cast<const float4*>(&slab[eb + 16 * s]);
            dn[1] = *reinterpret_cast<const float4*>(&slab[ob + 16 * s]);
            dn[2] = *reinterpret_cast<const float4*>(&slab[eb + WN_SLD + 16 * s]);
            dn[3] = *reinterpret_cast<const float4*>(&slab[ob + WN_SLD + 16 * s]);
            dn[4] = *reinterpret_cast<const float4*>(&slab[eb + 2 * WN_SLD + 16 * s]);
            Wino23Frag<NV> fr[2];
            read_frag(fr[0], Bc, s == 2);
            float v[5][4], vt[5];
            {
                const float d[5][4] = {{dn[0].x, dn[0].y, dn[0].z, dn[0].w}, {dn[1].x, dn[1].y, dn[1].z, dn[1].w}, {dn[2].x, dn[2].y, dn[2].z, dn[2].w},
                                       {dn[3].x, dn[3].y, dn[3].z, dn[3].w}, {dn[4].x, dn[4].y, dn[4].z, dn[4].w}};
#pragma unroll
                for (int i = 0; i < 4; ++i) wino_bt(d[0][i], d[1][i], d[2][i], d[3][i], d[4][i], v[0][i], v[1][i], v[2][i], v[3][i], v[4][i]);
            }
            if (s == 2) {
                const int te = eb - 4 * kq + 48 + kq, to = ob - 4 * kq + 48 + kq;
                wino_bt(slab[te], slab[to], slab[te + WN_SLD], slab[to + WN_SLD], slab[te + 2 * WN_SLD], vt[0], vt[1], vt[2], vt[3], vt[4]);
            }
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                const Wino23Frag<NV>& fg = fr[j & 1];
                if (j < 4) read_frag(fr[(j + 1) & 1], Bc + (j + 1) * WN_BTILE, s == 2);
                if (XSQ_WINO_SCHED2 >= 0) __builtin_amdgcn_sched_barrier(XSQ_WINO_SCHED2);
                const float wa[4] = {fg.w[0].x, fg.w[0].y, fg.w[0].z, fg.w[0].w}, wb[4] = {fg.w[1].x, fg.w[1].y, fg.w[1].z, fg.w[1].w};
                const float wc[4] = {fg.w[2].x, fg.w[2].y, fg.w[2].z, fg.w[2].w};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    acc[j][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[i], v[j][i], acc[j][0], 0, 0, 0);
                    acc[j][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(wb[i], v[j][i], acc[j][1], 0, 0, 0);
                    acc[j][2] = __builtin_amdgcn_mfma_f32_16x16x4f32(wc[i], v[j][i], acc[j][2], 0, 0, 0);
                }
                if (s == 2) {
                    acc[j][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(fg.wt[0], vt[j], acc[j][0], 0, 0, 0);
                    acc[j][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(fg.wt[1], vt[j], acc[j][1], 0, 0, 0);
                    acc[j][2] = __builtin_amdgcn_mfma_f32_16x16x4f32(fg.wt[2], vt[j], acc[j][2], 0, 0, 0);
                }
#pragma unroll
                for (int cc = 0; cc < NV; ++cc) {
                    asm("v_fmac_f32_dpp %0, %1, %2 row_newbcast:0 row_mask:0xf bank_mask:0xf\n\t"
                        "v_fmac_f32_dpp %0, %1, %3 row_newbcast:1 row_mask:0xf bank_mask:0xf\n\t"
                        "v_fmac_f32_dpp %0, %1, %4 row_newbcast:2 row_mask:0xf bank_mask:0xf\n\t"
                        "v_fmac_f32_dpp %0, %1, %5 row_newbcast:3 row_mask:0xf bank_mask:0xf"
                        : "+v"(accv[j][cc])
                        : "v"(fg.u[cc]), "v"(v[j][0]), "v"(v[j][1]), "v"(v[j][2]), "v"(v[j][3]));
                    if (s == 2) asm("v_fmac_f32 %0, %1, %2" : "+v"(accv[j][cc]) : "v"(vt[j]), "v"(fg.ut[cc]));
                }
                if (XSQ_WINO_SCHED >= 0) __builtin_amdgcn_sched_barrier(XSQ_WINO_SCHED);
            }
            // other buffer: last read in the chunk before, every wave is past that chunk's barrier
            if (s < 2) store_chunk(s + 1, cur ^ 1);
            else if (!last) store_chunk(0, cur ^ 1);
            cnt += 1;
            __syncthreads();
        }
    };

    // output transform, shift + ReLU of the lane's own pair (the epilogue of cdae_wino_kernel): accumulator register r is output
    // channel 16 cb + 4 kq + r; the vector columns' four k-quad sums meet in a fixed order
    auto outputs_main = [&](const float* shift, int cb, float4& o0, float4& o1) {
        const float4 sh = *reinterpret_cast<const float4*>(shift + 16 * cb + 4 * kq);
        const float shv[4] = {sh.x, sh.y, sh.z, sh.w};
        float y0[4], y1[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float m0 = acc[0][cb][r], m1 = acc[1][cb][r], m2 = acc[2][cb][r], m3 = acc[3][cb][r], m4 = acc[4][cb][r];
            y0[r] = fmaxf(((m0 + m1) + (m2 + m3)) + shv[r], 0.f);
            y1[r] = fmaxf((fmaf(2.f, m3, m1 - m2) + m4) + shv[r], 0.f);
        }
        o0 = make_float4(y0[0], y0[1], y0[2], y0[3]);
        o1 = make_float4(y1[0], y1[1], y1[2], y1[3]);
    };
    auto outputs_vec = [&](auto nv_, const float* shift, float4& o0, float4& o1) {
        constexpr int NV = decltype(nv_)::value;
        float y0v[4] = {0.f, 0.f, 0.f, 0.f}, y1v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int cc = 0; cc < NV; ++cc) {
            float m[5];
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                float x = accv[j][cc];
                x += __shfl_xor(x, 16);
                x += __shfl_xor(x, 32);
                m[j] = x;
            }
            y0v[cc] = ((m[0] + m[1]) + (m[2] + m[3]));
            y1v[cc] = fmaf(2.f, m[3], m[1] - m[2]) + m[4];
        }
        const float4 sh = *reinterpret_cast<const float4*>(shift + 48);
        o0 = make_float4(fmaxf(y0v[0] + sh.x, 0.f), fmaxf(y0v[1] + sh.y, 0.f), fmaxf(y0v[2] + sh.z, 0.f), fmaxf(y0v[3] + sh.w, 0.f));
        o1 = make_float4(fmaxf(y1v[0] + sh.x, 0.f), fmaxf(y1v[1] + sh.y, 0.f), fmaxf(y1v[2] + sh.z, 0.f), fmaxf(y1v[3] + sh.w, 0.f));
    };

    // ---- stage 1: act2 pairs A - 2 .. A + 61 from the act1 slab, written over the planes (free: the loop ended on a barrier)
    run_layer(std::integral_constant<int, H2 - 48>{}, std::false_type{}, ru2);
    {
        const float* shift = a.pool + t.shift2_off;
        const int t2 = 2 * (A - 2 + pl);                         // act2 position of output 0
        const bool in0 = (unsigned)t2 < (unsigned)T2, in1 = (unsigned)(t2 + 1) < (unsigned)T2;
        auto keep = [](bool in, const float4& o) { return make_float4(in ? o.x : 0.f, in ? o.y : 0.f, in ? o.z : 0.f, in ? o.w : 0.f); };
        float* d0 = slab + PLANE_O + (pl - 1) * WN_SLD;          // output 0: local position 2 pl - 1
        float* d1 = slab + pl * WN_SLD;                          // output 1: local position 2 pl
#pragma unroll
        for (int cb = 0; cb < 3; ++cb) {
            float4 o0, o1;
            outputs_main(shift, cb, o0, o1);
            if (pl > 0) *reinterpret_cast<float4*>(d0 + 16 * cb + 4 * kq) = keep(in0, o0);
            *reinterpret_cast<float4*>(d1 + 16 * cb + 4 * kq) = keep(in1, o1);
        }
        float4 o0, o1;
        outputs_vec(std::integral_constant<int, H2 - 48>{}, shift, o0, o1);
        if (kq == 0) {
            if (pl > 0) *reinterpret_cast<float4*>(d0 + 48) = keep(in0, o0);
            *reinterpret_cast<float4*>(d1 + 48) = keep(in1, o1);
        }
    }
    __syncthreads();

    // ---- stage 2: act3 pairs A .. A + 61 from those planes
    run_layer(std::integral_constant<int, H1 - 48>{}, std::true_type{}, ru3);
    {
        const float* shift = a.pool + t.shift3_off;
        const __amdgpu_buffer_rsrc_t ro = buf_rsrc(a.act3 + t.out_off, 0x40000000u);
        const int qq = A + pl;
        const bool ok0 = pl < WN23_OUT && 2 * qq < T1, ok1 = pl < WN23_OUT && 2 * qq + 1 < T1;
        const unsigned vo = 4u * (unsigned)((((b * F + f) * T1) + 2 * qq) * CS + 4 * kq);
#pragma unroll
        for (int cb = 0; cb < 3; ++cb) {
            float4 o0, o1;
            outputs_main(shift, cb, o0, o1);
            // (displacements in the LANE offset, scalar offset 0: the store-data hazard of 16-byte stores with an SGPR offset, common.h)
            buf_st4(o0, ro, ok0 ? vo + 64u * cb : BUF_OOB, 0);
            buf_st4(o1, ro, ok1 ? vo + 64u * cb + 4u * CS : BUF_OOB, 0);
        }
        float4 o0, o1;
        outputs_vec(std::integral_constant<int, H1 - 48>{}, shift, o0, o1);
        const unsigned vt48 = vo - 16u * (unsigned)kq;           // (channel 0 of the row)
        buf_st4(o0, ro, (ok0 && kq == 0) ? vt48 + 192u : BUF_OOB, 0);
        buf_st4(o1, ro, (ok1 && kq == 0) ? vt48 + 192u + 4u * CS : BUF_OOB, 0);
    }
}

}  // namespace xsq
