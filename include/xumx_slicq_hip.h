/*
 * xumx_slicq_hip.h -- C ABI of the MI355X (gfx950) demix hot path of xumx-sliCQ-V2.
 *
 * The reference (sevagh/xumx-sliCQ, branch v2) is pure Python/PyTorch and has no FFI
 * layer; its boundary for this path is the nn.Module surface of
 *   xumx_slicq_v2/transforms.py  (NSGT_SL.forward :106-131, INSGT_SL.forward :154-178)
 *   xumx_slicq_v2/model.py       (Unmix.forward :69-82, _SlicedUnmixCDAE.forward :213-271)
 *   xumx_slicq_v2/phase.py       (blockwise_wiener :18-69, blockwise_phasemix_sep :96-113)
 *   xumx_slicq_v2/separator.py   (Separator.forward :133-232)
 * This library sits directly under the Python mirrors of those modules
 * (xumx_slicq_amd/ *.py bind it with ctypes; INTEGRATION.md shows the stub a maintainer
 * of the reference would add).  Each entry point names the reference code it replaces.
 *
 * Conventions
 *  - plain C: pointers and sizes only; no torch types.
 *  - every data pointer is DEVICE memory owned by the caller (tensor.data_ptr() of a
 *    contiguous fp32 tensor); the library never frees caller memory.
 *  - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream).
 *    Calls are asynchronous on that stream; nothing synchronises the device.
 *  - return value: 0 on success, negative XSQ_ERR_* otherwise; xsq_last_error() gives
 *    the message of the calling thread's last failure.  Nothing throws across the ABI.
 *  - a plan / model is immutable after creation; workspaces are per call, so one plan
 *    can serve several streams as long as each call has its own workspace.
 *
 * Coefficient arena ("ragged blocks in one allocation")
 *  The sliCQT of `BC` packed channels with `S` slices is ONE fp32 buffer holding the
 *  reference's list of per-block tensors back to back: block b (F_b bins x T_b
 *  coefficients per slice) starts at float offset 2*BC*S*cum_b, cum_b = sum_{b'<b} F_b'*T_b',
 *  and is laid out (BC, F_b, S, T_b, 2) contiguous -- exactly the tensor
 *  NSGT_SL.forward returns for that block, so Python exposes views, not copies.
 *  xsq_plan_block_table() returns (first_band, F_b, T_b, cum_b) per block.
 */
#ifndef XUMX_SLICQ_HIP_H
#define XUMX_SLICQ_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define XSQ_ABI_VERSION 2   /* 2 (round 5): xsq_exchange_rows takes the buffer lengths; *_indirect entry points */

typedef struct xsq_plan xsq_plan;
typedef struct xsq_model xsq_model;

/* ---- library ---------------------------------------------------------------- */
int xsq_abi_version(void);
const char* xsq_last_error(void);
/* How this library was built: "arch=<offload arch>; flags=<the Makefile's EXTRA and NOPK>; date=<__DATE__ __TIME__>" -- a
 * diagnostic build (ablation / stamp macros) says so here, and bench.py copies the string into its JSON line. */
const char* xsq_build_info(void);

/* ---- sliCQT plan ---------------------------------------------------------------
 * Replaces the plan objects built by NSGT_sliced.__init__ (nsgt/slicq.py:70-151):
 * window lengths M / windows g (nsgt/nsgfwin_sl.py:8-111), centre bins and index
 * ranges (nsgt/util.py:72-100), dual windows gd (nsgt/util.py:103-116), slice window
 * (nsgt/slicing.py:7-18).  The host computes those tables (xumx_slicq_amd/plan.py);
 * this call uploads them and builds the per-band DFT matrices.
 *   Lg[nbands], c[nbands]   band lengths and centre bins (bands DC..Nyquist)
 *   g   concatenated analysis windows (sum Lg floats), peak at index 0 of each band
 *   gd  concatenated dual windows (sum Lg doubles), same order
 *   tw  slice (Tukey) window, L floats                                               */
int xsq_plan_create(xsq_plan** out, int L, int tr, int nbands, const int32_t* Lg,
                    const int32_t* c, const float* g, const double* gd, const float* tw);

/* What the inverse transforms of this library leave out of the reference's on a plan of xsq_plan_create
 * (nsgt/nsigtf.py:57-99): the second synthesis of a band that reaches across DC (0 < c_j < Lg_j/2) through its negative-frequency mirror.  share[nbands] = the weight of that
 * term relative to the band's kept synthesis (0 for a band that does not cross DC), *worst (may be null) the band of the
 * largest.  Host arithmetic, no device.  xsq_plan_create returns XSQ_ERR_ARG, naming the band, for a plan with a share of
 * XSQ_TWIN_SHARE_MAX or more: Bark-262 has no such band, Mel-32 one of 0.0084; `bark, 96, 32.9` (0.109) is refused.   */
#define XSQ_TWIN_SHARE_MAX 0.03
int xsq_slicqt_dropped_twin_share(int L, int nbands, const int32_t* Lg, const int32_t* c, const double* gd, double* share,
                                  int* worst);
/* xsq_plan_create with that term computed instead (opt-in; build_plan(dc_twins=True)): never refuses for a band across DC.
 * The table of the term -- band j with 0 < c_j < Lg_j/2 lands on bin q - c_j, c_j <= q < Lg_j/2, with the weight
 * (-1)^(c_j/2) (-1)^q Lg_j gd_j[Lg_j - q] -- is derived here from Lg, c and gd and uploaded.  Every inverse without a carry
 * (xsq_slicqt_inverse{,_rows,_masked,_remix}, and through them xsq_separator_forward and xsq_ideal_separate) then adds it to the
 * slice spectra (k_twin_synthesis), and xsq_slicqt_inverse_adjoint its transpose (k_twin_analysis).  Such a plan always takes
 * the rocFFT path, and xsq_slicqt_inverse_masked_carry (streaming) refuses it.  A plan without such a band behaves exactly
 * like xsq_plan_create's.  xsq_plan_num_twins: the number of landing entries (8 for `bark, 28, 32.9`), 0 for any plan of
 * xsq_plan_create.                                                                                                  */
int xsq_plan_create_twins(xsq_plan** out, int L, int tr, int nbands, const int32_t* Lg,
                          const int32_t* c, const float* g, const double* gd, const float* tw);
int xsq_plan_num_twins(const xsq_plan* plan);
/* xsq_plan_create with options (XSQ_ABI_VERSION stays 2: more exports).  flags = 0 is xsq_plan_create, XSQ_PLAN_TWINS is
 * xsq_plan_create_twins.  XSQ_PLAN_LONG_BANDS (build_plan(long_bands=True)): every band with Lg above xsq_plan_long_band_min()
 * (320) runs on the FFT band engine (csrc/band_fft.h: one radix-4 split and a chirp-z transform of length Lg / 4 through a
 * power-of-two FFT in LDS; O(Lg log Lg) work, tables linear in Lg) instead of the dense engine, whose matrices are quadratic in
 * Lg -- the upper bands of the logarithmic scales (`cqlog, 12, 20.0`: Lg up to 6416).  Both transforms, both adjoints and the
 * masked and remix inverses use it; xsq_slicqt_forward_xin and its _rows / _rows_indirect / _ring forms serve such a plan (the
 * engine's analysis writes the whitened magnitude of its bands beside the coefficients, in the layout and the split-bf16 format
 * of the other engines: the network runs on one), and such a plan takes the rocFFT path.  A band longer than xsq_plan_long_band_max() (16384) is refused by
 * name (XSQ_ERR_ARG).  A plan without a band above 320 behaves exactly like that of the other flags alone.
 * xsq_plan_num_long_bands: the bands on the engine, 0 for a plan without the flag.                                    */
#define XSQ_PLAN_TWINS 1u
#define XSQ_PLAN_LONG_BANDS 2u
int xsq_plan_create_flags(xsq_plan** out, int L, int tr, int nbands, const int32_t* Lg,
                          const int32_t* c, const float* g, const double* gd, const float* tw, unsigned flags);
int xsq_plan_long_band_max(void);
int xsq_plan_long_band_min(void);
int xsq_plan_num_long_bands(const xsq_plan* plan);
int xsq_plan_destroy(xsq_plan* plan);
int xsq_plan_num_blocks(const xsq_plan* plan);
/* slice-FFT backend: 0 (default) = the hand-written LDS-resident transform when L == 18060
 * (the Bark-262 plan of both pretrained models), rocFFT otherwise; 1 = always rocFFT.     */
int xsq_plan_set_fft_backend(xsq_plan* plan, int backend);
/* per-band DFTs: 1 (default) = bands with Lg >= 24 (163 of the 263 Bark-262 bands, 99 % of the band-DFT flops; the split
 * point XSQ_D4_MIN_LG_DEFAULT of csrc/slicqt.hip) run on the radix-4 kernel (one decimation-in-
 * frequency stage fused into the operand staging, 4x fewer MFMA flops); 0 = all bands on the
 * dense grouped GEMM.                                                                      */
int xsq_plan_set_band_radix4(xsq_plan* plan, int on);
/* inverse transform, bands below the radix-4 split (Lg < 24: 100 of the 263 Bark-262 bands): 0 (default) = on the dense grouped GEMM;
 * 1 = synthesised inside the inverse slice-FFT kernel straight from the coefficients (radix-4 stage + 4..15-point
 * codelets, no Z round trip, no dense DFT-matrix GEMM) -- an experiment that measured 0.03-0.05 ms SLOWER per 240 s
 * track (the kernel is bound by its chain of memory / LDS round trips) and is kept as an A/B switch.  Ignored
 * when the plan is not eligible (rocFFT backend, other band lengths).                                       */
int xsq_plan_set_short_inline(xsq_plan* plan, int on);
/* hand-written slice FFT only: 1 = its 43 / 14 / 15-point butterflies on packed-fp32 vector instructions (v_pk_fma_f32
 * on the (re, im) register pair: half the vector instructions, bitwise the same results).  DIAGNOSTIC builds only
 * (csrc/Makefile PACKED_FFT=1): the product library does not contain those kernels and returns XSQ_ERR_ARG for on != 0 --
 * a packed-fp32 transform next to v_mfma_f32_16x16x32_bf16 waves of another stream returned wrong values on MI355X
 * (tools/probe/pk_mfma_hazard.hip), which no guard at this level can exclude, and it measured no
 * faster.                                                                                                       */
int xsq_plan_set_packed_fft(xsq_plan* plan, int on);
/* table: nblocks x 4 int64 (first_band, F_b, T_b, cum_b) */
int xsq_plan_block_table(const xsq_plan* plan, int64_t* table);
/* complex coefficients per channel-slice (sum_b F_b*T_b) */
int64_t xsq_plan_coefs_per_slice(const xsq_plan* plan);
/* slices of an n-sample signal (nsgt/slicing.py:47-72): floor((ceil(n/h)+1)/2)+1 */
int xsq_plan_num_slices(const xsq_plan* plan, int64_t n);

/* ---- forward sliCQT -----------------------------------------------------------
 * Replaces NSGT_SL.forward (transforms.py:106-131) -> NSGT_sliced.forward
 * (nsgt/slicq.py:182-196): slicing+Tukey (nsgt/slicing.py:21-72), L-point FFT and
 * per-band window * gather * IFFT (nsgt/nsgtf.py:7-84), arrange (nsgt/slicq.py:13-33).
 *   x     (BC, n) fp32 packed channels        coef  arena for BC channels, S slices  */
size_t xsq_slicqt_forward_workspace(xsq_plan* plan, int BC, int64_t n);   /* 0 on error */
int xsq_slicqt_forward(xsq_plan* plan, const float* x, int BC, int64_t n, float* coef,
                       void* workspace, size_t workspace_bytes, void* stream);
/* The same transform, with the CDAE's whitened input written beside the coefficients by the analysis kernels'
 * epilogues: xin[i] = (|coef[i]| + mean[band]) * scale[band] (model.py:238-242; Unmix.forward's abs_of_real_complex,
 * model.py:74-76), real arena layout for BC channels -- normally the head of the xsq_cdae_forward workspace, with
 * mean / scale / split from xsq_model_whitening; xsq_cdae_forward_xin(..., xin_ready = 1) then skips its magnitude
 * pass (one kernel and a second read of the 87 MB mix arena less per chunk).  xin == NULL: plain forward.     */
int xsq_slicqt_forward_xin(xsq_plan* plan, const float* x, int BC, int64_t n, float* coef, float* xin,
                           const float* mean, const float* scale, int split,
                           void* workspace, size_t workspace_bytes, void* stream);

/* The same transform reading packed channel r at x + x_row_offsets[r] (DEVICE array of BC int64 element offsets; NULL =
 * r * n): the chunks of a (nb_samples, 2, N) track that Separator.forward stacks along the batch axis are read where
 * they lie (the reference slices views too, separator.py:153-158) instead of through a packing copy.  n = samples that
 * exist per row, n_pad >= n = the length the slice count is taken from: the zero padding of a short last chunk to
 * sllen/2 + 1 samples (separator.py:162-168) without materialising the zeros (the kernels read zeros outside [0, n)). */
int xsq_slicqt_forward_rows(xsq_plan* plan, const float* x, const int64_t* x_row_offsets, int BC, int64_t n,
                            int64_t n_pad, float* coef, float* xin, const float* mean, const float* scale, int split,
                            void* workspace, size_t workspace_bytes, void* stream);
/* The same call with the input's base pointer read from DEVICE memory when the kernel runs: x_slot != NULL -> the rows
 * start at *x_slot + x_row_offsets[r] (x is then ignored and may be NULL).  A HIP graph captured around the call follows
 * whatever tensor the caller points the slot at before each replay (an 8-byte device write) -- the graphed form of the
 * `separator(audio)` call timed at inference.py:28-31 needs no copy of the input into a static buffer.               */
int xsq_slicqt_forward_rows_indirect(xsq_plan* plan, const float* x, const float* const* x_slot, const int64_t* x_row_offsets,
                                     int BC, int64_t n, int64_t n_pad, float* coef, float* xin, const float* mean,
                                     const float* scale, int split, void* workspace, size_t workspace_bytes, void* stream);

/* ---- inverse sliCQT -----------------------------------------------------------
 * Replaces INSGT_SL.forward (transforms.py:154-178) -> NSGT_sliced.backward
 * (nsgt/slicq.py:198-230): per-band FFT, dual-window multiply and overlap-add into the
 * slice spectrum (nsgt/nsigtf.py:5-106), irfft, un-rotate + overlap-add of slices
 * (nsgt/unslicing.py:6-69), crop to `length`.  Does NOT modify `coef` (the reference
 * decoder overwrites its input).
 *   coef  arena for BC channels, S slices     y  (BC, length) fp32                    */
size_t xsq_slicqt_inverse_workspace(xsq_plan* plan, int BC, int S);       /* 0 on error */
int xsq_slicqt_inverse(xsq_plan* plan, const float* coef, int BC, int S, int64_t length,
                       float* y, void* workspace, size_t workspace_bytes, void* stream);
/* Same, but packed channel r is written at y + row_offsets[r] (DEVICE array of BC int64 element
 * offsets) instead of y + r*length: lets the caller place every chunk's stems directly in the
 * final (4, nb_samples, 2, N) tensor -- the torch.cat of separator.py:231 without the copy.   */
int xsq_slicqt_inverse_rows(xsq_plan* plan, const float* coef, int BC, int S, int64_t length,
                            float* y, const int64_t* row_offsets, void* workspace,
                            size_t workspace_bytes, void* stream);
/*   The separator's mix-phase path without the intermediate estimate arena: the coefficients of
 *   packed channel bc are masks[bc] * mix[bc % BCx], formed while the band DFT loads them
 *   (phase.py:96-113 fused into nsigtf.py:85-95).  masks: REAL arena, BC channels (what
 *   xsq_cdae_forward writes with Y = NULL); mix: complex arena, BCx channels.               */
int xsq_slicqt_inverse_masked(xsq_plan* plan, const float* masks, const float* mix, int BC, int BCx,
                              int S, int64_t length, float* y, const int64_t* row_offsets,
                              void* workspace, size_t workspace_bytes, void* stream);
/*   R gain-weighted mixes of the four targets through R inverse transforms instead of four plus a sum: the
 *   slider mix of demixui.py:94-114 (sum_t level_t * stem_t), remix_signal of cadenza/enhance.py:270-290 and the
 *   target groups of separator.py:235-259 (to_dict with aggregate_dict).  The inverse is linear, so
 *     mix-phase:  sum_t g_t iSliCQT(m_t * X) = iSliCQT((sum_t g_t m_t) * X)
 *     Wiener-EM:  sum_t g_t iSliCQT(Y_t)     = iSliCQT(sum_t g_t Y_t)
 *   A combine kernel forms the weighted masks (real) or estimates (complex) of the R mixes, t = 0..3 in this order with
 *   the products rounded before the sum (a one-hot row reproduces its target bit for bit), skipping every target no row
 *   weights; then xsq_slicqt_inverse_masked / xsq_slicqt_inverse_rows runs on R * 2B channels.
 *   Mix-phase: masks = REAL arena of 8B channels (target, item, c), mix = complex arena of 2B channels, Y = NULL.
 *   Wiener-EM: Y = complex arena of 8B channels, masks = mix = NULL.  gains: HOST float[R * 4], row-major, targets in
 *   Separator.sources order (bass, vocals, other, drums), finite; 1 <= R <= 4.  Output channel (r, item, c) -> y +
 *   row_offsets[r * 2B + 2 item + c] (row_offsets: DEVICE int64[R * 2B], NULL: contiguous rows of `length`).
 *   workspace: xsq_slicqt_remix_workspace bytes (wiener = Y != NULL).                                                  */
size_t xsq_slicqt_remix_workspace(xsq_plan* plan, int R, int B, int S, int wiener);      /* 0 on error */
int xsq_slicqt_inverse_remix(xsq_plan* plan, const float* masks, const float* mix, const float* Y, const float* gains,
                             int R, int B, int S, int64_t length, float* y, const int64_t* row_offsets,
                             void* workspace, size_t workspace_bytes, void* stream);

/* ---- CDAE model ----------------------------------------------------------------
 * Replaces Unmix.forward (model.py:69-82) -> _SlicedUnmixCDAE.forward (model.py:213-271)
 * for all blocks and the four targets, with the mix-phase estimate
 * blockwise_phasemix_sep (phase.py:96-113; == mask * X) fused into
 * the last layer.  The Wiener-EM refinement is xsq_wiener_em below.
 *
 * `params` is a HOST buffer: the fp32 tensors of the reference state_dict in its own
 * key order (per block: input_mean, input_scale; per target: 0.weight, 1.{weight,bias,
 * running_mean,running_var}, 3.weight, 4.{...}, 6.weight, 7.{...}, 9.weight, 9.bias),
 * num_batches_tracked left out.  BatchNorm (eval) is folded at creation.
 * `causal` != 0 selects _CausalConv2d for layer 1 (model.py:274-290).  The block table
 * (F_b bins, T_b coefficients per slice) is the one Unmix receives through its
 * jagged_slicq_sample_input (model.py:29-57); kf follows model.py:112-117.               */
int64_t xsq_model_num_params(int nblocks, const int32_t* F, const int32_t* T);
int xsq_model_create(xsq_model** out, int nblocks, const int32_t* F, const int32_t* T,
                     int causal, const float* params, int64_t nparams);
int xsq_model_destroy(xsq_model* model);
/* Arithmetic of the four convolution layers (the contraction only; epilogues, BatchNorm folding,
 * sigmoid and every other kernel of the path stay fp32).  Inference only.
 *   0  fp32 operands on v_mfma_f32_32x32x2_f32 (default; what the parity fixtures were pinned with)
 *   1  "bf16x3": every fp32 operand carried as hi + lo bf16, three bf16 MFMAs per product, fp32
 *      accumulation -- ~2^-17 relative per product (finer than the TF32 convolutions the
 *      reference's torch-cuda backend runs by default, model.py:130-181 under
 *      torch.backends.cudnn.allow_tf32), 3/16 of the matrix-pipe time.
 *   2  "bf16x6": every fp32 operand cut EXACTLY into three bf16 pieces, the six partial products of
 *      weight >= 2^-16 on bf16 MFMAs, fp32 accumulation; what is dropped is <= 2^-23 |ab| per
 *      product, one fp32 rounding -- measured as close to the torch-cpu reference as mode 0
 *      (1.1e-7 RMS), 6/16 of the matrix-pipe time.                                              */
int xsq_model_set_precision(xsq_model* model, int mode);
/* Fast-convolution forms of the fp32 inference layers, a bit mask (default 7 = bits 1, 2 and 4):
 *   1  layers 2 / 3 (the 4-tap time convolutions of model.py:140-170), rows of >= 127 time positions: Winograd F(2, 4) along
 *      the time taps (csrc/cdae_wino.h: five MFMA products per output pair and channel pair instead of eight; input transform
 *      with integer coefficients in registers, weights transformed on the host in fp64; ~2e-7 RMS of a layer's output against
 *      fp64 where the direct fp32 sum has ~7e-8).  Without the bit: the direct slab kernels (csrc/cdae_slab.h).
 *   2  layer 1 (model.py:130-139, non-causal): F(2, 2) along the hop (csrc/cdae_l1f.h: the strided (kf, W) convolution is a
 *      two-tap convolution in units of the hop -- three half-window products per output pair instead of four, W0 + W1 summed
 *      on the host in fp64).  Without the bit: the implicit GEMM (CdaeL1Op).
 *   4  layer 4 (model.py:171-181, non-causal): F(2, 2) along the hop the same way (csrc/cdae_l4f.h), masks only or with the
 *      estimates materialised.  Without the bit: the implicit GEMM (CdaeL4Op).
 *   8  (with bit 1) layers 2 / 3, rows of >= 253 time positions: Winograd F(4, 4) (csrc/cdae_wino4.h: seven products per
 *      output quad instead of ten).  An A/B arm, off by default: parity-green and measured 8-10 % slower than F(2, 4) on
 *      MI355X.  Its weights are built only into models created with XSQ_WINO4=1 in the environment; the bit is an error on
 *      any other model.
 *  16  (with bit 1) layers 2 and 3 of the blocks with ONE frequency tap in one launch where both layers run F(2, 4) (rows of
 *      layer 2 of >= 127 positions too): layer 2's output stays in LDS (csrc/cdae_wino23.h).  Bit for bit the result of the two
 *      launches.  On by default: the default mask is 23.
 * The split-bf16 modes, the causal first layer and (bits 1, 8) shorter rows always take the direct kernels.              */
int xsq_model_set_winograd(xsq_model* model, int on);
size_t xsq_cdae_workspace(const xsq_model* model, int B, int S);          /* 0 on error */
/*   X      mix coefficients, arena for 2*B channels (B, 2, ...)
 *   Y      out: mask * X, arena for 8*B channels laid out (4 targets, B, 2, ...); NULL (with masks
 *          given) writes the masks only -- the input xsq_slicqt_inverse_masked expects
 *   masks  out, optional (NULL to skip): sigmoid masks, REAL arena with the geometry of Y
 *          (one float per coefficient) -- Unmix.forward(return_masks=True)             */
int xsq_cdae_forward(xsq_model* model, const float* X, int B, int S, float* Y, float* masks,
                     void* workspace, size_t workspace_bytes, void* stream);
/* xin_ready != 0: the head of `workspace` (2 B S sum(F T) floats) already holds the whitened magnitude, written by
 * xsq_slicqt_forward_xin with this model's tables (xsq_model_whitening: device pointers to input_mean / input_scale
 * per band and the operand format of the current precision mode).                                            */
int xsq_cdae_forward_xin(xsq_model* model, const float* X, int B, int S, float* Y, float* masks,
                         void* workspace, size_t workspace_bytes, void* stream, int xin_ready);
int xsq_model_whitening(xsq_model* model, const float** mean, const float** scale, int* split);

/* ---- post-filters on the arena ---------------------------------------------------
 * Both take an explicit block table (nblocks, F[], T[]) so that they also serve the
 * reference's single-block helpers (phase.py) on shapes outside the sliCQT plan.
 *
 * xsq_phasemix replaces blockwise_phasemix_sep (phase.py:96-113, with _atan2 :72-93):
 *   Y[j,b,c] = mag[j,b,c] * X[b,c] / |X[b,c]|   (angle(0) := 0); does not modify X
 *   (the reference's _atan2 adds 1 to re(X) where X == 0).
 *   The unit phase is exact to fp32 rounding for EVERY finite non-zero X: where re^2 + im^2 is not a normal
 *   fp32 number (|X| below about 1.1e-19 or above 1.8e19) X is divided by max(|re|, |im|) before it is
 *   normalised; elsewhere the plain form, bit for bit what earlier versions returned.
 *   X  complex arena, 2*B channels;  mag  REAL arena, 8*B channels (4, B, 2, ...);
 *   Y  complex arena, 8*B channels.
 *
 * xsq_wiener_em replaces blockwise_wiener (phase.py:18-69) after the initial estimate:
 * norbert.wiener(v, x, iterations=1, use_softmask=False) (norbert/__init__.py:153-260)
 * per window of <= win_len frames of the flattened (slice, time) axis.
 *   X  complex arena, 2*B channels
 *   Y  in: initial estimates y0 = v * exp(i angle x) (what xsq_cdae_forward / xsq_phasemix
 *      write); out: refined estimates, in place.                                        */
int xsq_phasemix(int nblocks, const int32_t* F, const int32_t* T, const float* X,
                 const float* mag, float* Y, int B, int S, void* stream);
size_t xsq_wiener_workspace(int nblocks, const int32_t* F, const int32_t* T, int B, int S,
                            int win_len);                                   /* 0 on error */
/*   batch_group: the window maximum max(1, 0.1*max|x|) of norbert :257 spans the batch dimension
 *   (SURVEY.md quirk A13).  <= 0 or B: one group, the reference's behaviour for one call.  g < B
 *   (g divides B): every run of g consecutive batch items is its own group -- lets a caller stack
 *   independent chunks along the batch axis without changing any chunk's result.          */
int xsq_wiener_em(int nblocks, const int32_t* F, const int32_t* T, const float* X, float* Y,
                  int B, int S, int win_len, int batch_group, void* workspace,
                  size_t workspace_bytes, void* stream);

/* ---- placement of packed stems (sharded path) -------------------------------------------------
 * Replaces the hard torch.cat of separator.py:229-231 for stems that were computed on OTHER ranks and arrive packed
 * in an all-gather buffer (xumx_slicq_amd/sharding.py): row i of the table is copied as
 *   dst[table[3i+1] : + table[3i+2]] = src[table[3i] : + table[3i+2]]      (float offsets / lengths)
 * in ONE launch for all rows (item x target x sample x channel) of an exchange.  table: DEVICE int64[nrows][3];
 * max_len = the largest row length (sizes the grid).  Rows must not overlap in dst.                     */
int xsq_place_rows(const float* src, float* dst, const int64_t* table, int nrows, int64_t max_len, void* stream);

/* ---- sample-rate conversion of the front end ---------------------------------------------------------------------
 * Replaces torchaudio.transforms.Resample(orig, new, "sinc_interpolation") of data.py:148-156 (preprocess_audio): Hann
 * window, the polyphase filter torchaudio applies as conv1d(x_pad, K, stride o) with o = orig / g, n = new / g,
 * g = gcd(orig, new).  The host (xumx_slicq_amd/resample.py) builds K and keeps only each phase's non-zero taps:
 *   table      DEVICE fp32 [n][span]: K[p][first_tap[p] + i], i < span (zeros past a phase's last non-zero tap)
 *   first_tap  DEVICE int32 [n]: index k of table[p][0] in K's 2*width + o taps
 * and row r of y (rows rows, y + r * y_stride) becomes
 *   y[j*n + p] = sum_{i < span} table[p][i] * x[j*o + first_tap[p] - width + i],   j*n + p < len_out
 * summed in that order, where x (x + r * x_stride, len_in samples) reads as 0 outside [0, len_in) -- torchaudio's
 * padding, never written out.  len_out: ceil(fp32(n * len_in / o)), as torchaudio.  All offsets must fit 32 bits.
 * No allocation, no synchronisation: capturable into a graph.                                                     */
int xsq_resample(const float* x, int64_t x_stride, int rows, int64_t len_in, float* y, int64_t y_stride, int64_t len_out,
                 const float* table, const int32_t* first_tap, int o, int n, int span, int width, void* stream);

/* ---- one training batch from the device-resident stems ---------------------------------------------------------------
 * Replaces MUSDBDataset.__getitem__ with random_track_mix (data.py:316-390: per source a random track, an excerpt,
 * `audio * g` of data.py:183-188, the channel flip of data.py:191-196, torch.stack + stems.sum(0) of data.py:362-364) and
 * the DataLoader's collate of B items, for stems that stay on the device (xumx_slicq_amd/data.py).  ONE launch per step.
 *   pool     DEVICE, 16-byte aligned; fp32 (XSQ_POOL_FP32) or the files' int16 (XSQ_POOL_PCM16, value / 32768).  A track is
 *            8 rows of `len` samples, row (source column s, channel c) at element tracks[2t] + (2s + c) * round_up(len, 8):
 *            every row starts 16-byte aligned in both dtypes.
 *   tracks   DEVICE int64 [ntracks][2]: element offset of the track's first row (a multiple of 8), len in samples
 *   draws    DEVICE int32 [nsteps][B][4 source columns][4]: track, start, gain (fp32 bits), swap (0 / 1); `step` picks
 *            the B records of this launch.  The table is trusted, as row_offsets of xsq_crossfade_place is: the caller
 *            guarantees 0 <= track < ntracks and 0 <= start, and start + n <= len unless the track is shorter than n.
 *   target_of_column  DEVICE int32 [4]: the plane of y that source column s lands in
 * With v = the pool sample of track t(b, s), channel c ^ swap(b, s), at start(b, s) + i (0 where start + i >= len: a short
 * track is zero-padded at its tail; pcm16 converts exactly, float(int) * 2^-15):
 *   y[target_of_column[s], b, c, i] = fl32(gain(b, s) * v)                     y (4, B, 2, n) contiguous fp32
 *   x[b, c, i] = ((y_0 + y_1) + y_2) + y_3   in fp32, in source-column order   x (B, 2, n) contiguous fp32
 * The product is rounded BEFORE the sums (no fused multiply-add), as torch rounds `audio * g` before `stems.sum(0)`.
 * Every element of x and y is written exactly once; nothing is read at or past a row's len.  1 <= n < 2^31,
 * 1 <= B <= 32767.  No allocation, no synchronisation: capturable into a graph.                                       */
#define XSQ_POOL_FP32 0
#define XSQ_POOL_PCM16 1
int xsq_batch_assemble(const void* pool, int pool_dtype, const int64_t* tracks, int ntracks, const int32_t* draws,
                       int64_t step, int B, int64_t n, const int32_t* target_of_column, float* x, float* y, void* stream);

/* ---- in-place exchange of stems between the ranks of the sharded path (RCCL over xGMI) -------------------------------
 * The form of "the final waveform concat" (separator.py:229-231 across ranks) that needs no packing buffer and no
 * placement pass: every rank holds the SAME flat per-track layout, its kernels write the rows it owns in place
 * (xsq_demix_pass through out_rows), and ONE grouped ncclSend / ncclRecv per pass moves every row owner -> peers at
 * identical offsets -- point to point, one xGMI link per peer.
 *   xsq_comm_load       resolve RCCL from the library the process already uses (path of torch's librccl.so; NULL: by name)
 *   xsq_comm_unique_id  rank 0: 128 bytes to hand to every rank (torch.distributed broadcast)
 *   xsq_comm_create     ncclCommInitRank on the CURRENT device -- collective over the ranks
 *   xsq_exchange_rows   rows: HOST int64[nrows][4] = (owner rank, src float offset, dst float offset, length), the same
 *                       table on every rank; the owner sends src + src_off to every peer, every other rank receives into
 *                       dst + dst_off (src == dst and equal offsets: in place).  src_len / dst_len: floats behind src / dst --
 *                       every row's spans are checked against them before anything is queued.  Grouped ncclSend / ncclRecv
 *                       on `stream`, asynchronous; a group is closed every XSQ_EXCHANGE_GROUP_ROWS rows (default ~1024
 *                       point-to-point operations), at the same rows on every rank.  self_loop != 0 (tests, group of
 *                       one): the owner also sends to ITSELF and receives into dst -- src and dst must then not overlap. */
typedef struct xsq_comm xsq_comm;
int xsq_comm_load(const char* librccl_path);
int xsq_comm_version(void);                                                /* ncclGetVersion code, -1 on error */
int xsq_comm_unique_id(void* id128);
int xsq_comm_create(xsq_comm** out, const void* id128, int world, int rank);
int xsq_comm_destroy(xsq_comm* comm);
int xsq_comm_abort(xsq_comm* comm);                                        /* ncclCommAbort: do not wait for queued operations; frees the handle */
int xsq_exchange_rows(xsq_comm* comm, const float* src, int64_t src_len, float* dst, int64_t dst_len, const int64_t* rows,
                      int nrows, int self_loop, void* stream);

/* The same EM iteration fed by the MASKS (real arena, 8*B channels: what xsq_cdae_forward writes with Y = NULL): the
 * initial estimate y0 = mask * x (model.py:262-264 -> phase.py:96-113; == mask * X) is formed
 * while both passes load, so the CDAE's last layer stores 4 instead of 8 bytes per coefficient and the statistics pass
 * reads 48 instead of 80 bytes per time-frequency point.  Y is written only (refined estimates); same bits as
 * xsq_cdae_forward(Y) + xsq_wiener_em.  win_len and every S*T_b must be even (two frames per thread).       */
int xsq_wiener_em_masked(int nblocks, const int32_t* F, const int32_t* T, const float* X, const float* masks,
                         float* Y, int B, int S, int win_len, int batch_group, void* workspace,
                         size_t workspace_bytes, void* stream);

/* A batch too large for one pass (xsq_separator_forward splits it over the samples): the window maximum of norbert :257
 * spans the WHOLE batch, so every pass first folds the maxima of its samples into a shared table, and the EM of each pass
 * then takes max(own, table).  ext_max: DEVICE float[xsq_wiener_num_windows(...)], one entry per (block, group, window)
 * in block-major order, zeroed by the caller before the first xsq_wiener_window_max; holds max |x|^2.  Passes of one set
 * must agree on B / batch_group = number of groups.  ext_max == NULL: xsq_wiener_em_masked.                            */
int64_t xsq_wiener_num_windows(int nblocks, const int32_t* F, const int32_t* T, int B, int S, int win_len, int batch_group);
int xsq_wiener_window_max(int nblocks, const int32_t* F, const int32_t* T, const float* X, int B, int S, int win_len,
                          int batch_group, float* ext_max, void* stream);
int xsq_wiener_em_masked_ext(int nblocks, const int32_t* F, const int32_t* T, const float* X, const float* masks,
                             float* Y, int B, int S, int win_len, int batch_group, const float* ext_max,
                             void* workspace, size_t workspace_bytes, void* stream);

/* More than one EM iteration: norbert.wiener(v, x, iterations = niter, use_softmask=False), the `niter` of the Open-Unmix
 * family.  The reference's caller pins it to 1 (phase.py:53-58); norbert itself loops, norbert/__init__.py:133-148
 * (expectation_maximization: v and R are recomputed from the current estimates in every iteration) inside ONE scaling by
 * max(1, 0.1 max|x|) per window, norbert/__init__.py:247-260 (wiener).  Windows, batch_group and ext_max as above.
 *   niter   0: Y is the initial estimate (xsq_wiener_em_iter leaves it alone; the masked entry point refuses 0 -- the
 *              mix-phase estimate mask * X has no EM pass), 1: exactly the launches of xsq_wiener_em /
 *              xsq_wiener_em_masked_ext (same bits), >= 2: one of the two forms below.  Negative: XSQ_ERR_ARG.
 *   method  0 auto: resident when the longest window of the call fits, else looped; 1 looped: iteration 1 as above,
 *           then per iteration the statistics of the current estimates and the apply kernel in place on Y (any window
 *           length); 2 resident: one workgroup per (row, window) holds the window's frames on chip over all iterations
 *           -- one read of the inputs, one write of Y, whatever niter is -- for windows of at most
 *           xsq_wiener_resident_max_window() frames (>= the default 5000), XSQ_ERR_ARG when the call has a longer one.
 *   The two forms agree to fp32 rounding, not bitwise; each is bitwise reproducible (no atomics in the sums).
 *   workspace: xsq_wiener_iter_workspace bytes (0 on error).                                                            */
int xsq_wiener_resident_max_window(void);
size_t xsq_wiener_iter_workspace(int nblocks, const int32_t* F, const int32_t* T, int B, int S, int win_len, int niter,
                                 int method);
/* norbert/__init__.py:133-148, 247-260 on the estimates arena, in place (the many-iteration form of xsq_wiener_em). */
int xsq_wiener_em_iter(int nblocks, const int32_t* F, const int32_t* T, const float* X, float* Y, int B, int S,
                       int win_len, int batch_group, int niter, int method, void* workspace, size_t workspace_bytes,
                       void* stream);
/* norbert/__init__.py:133-148, 247-260 fed by the masks (the many-iteration form of xsq_wiener_em_masked_ext; ext_max
 * may be NULL).  win_len and every S*T_b must be even.                                                              */
int xsq_wiener_em_masked_iter(int nblocks, const int32_t* F, const int32_t* T, const float* X, const float* masks,
                              float* Y, int B, int S, int win_len, int batch_group, const float* ext_max, int niter,
                              int method, void* workspace, size_t workspace_bytes, void* stream);

/* ---- the other two post-filter options of the Open-Unmix family: softmask and the residual source ------------------------
 * norbert.wiener(v, x, niter, use_softmask=softmask) on v = contrib.residual_model(v, x, alpha=1) when residual is set
 * (norbert/__init__.py:247-248, :263-309; norbert/contrib.py:11-77), per window as above.  flags:
 *   XSQ_WIENER_SOFTMASK  the initial estimates are the ratio mask  y_j = x v_j / (eps + sum_j v_j)  per channel instead of the
 *                        mixture phase on v_j (sum over all sources, the residual included)
 *   XSQ_WIENER_RESIDUAL  a fifth source  v_4 = relu(max(|x|, eps) - sum_{j<4} v_j)  per channel: what the four targets do not
 *                        explain.  The estimates' arena then has 10*B channels (5, B, 2, ...), residual last, and the
 *                        statistics slot 32 floats (20 sums, max|x|^2, pad[3], 5 denominators, pad[3]); the masks' / magnitudes'
 *                        arena keeps 8*B.  The residual is formed from the mix and the four masks as a frame is loaded.
 * eps = FLT_EPSILON everywhere.  flags = 0 is the call without options, launch for launch.
 *   xsq_wiener_start              the J initial estimates from MAGNITUDES v (real arena, 8*B channels) into Y (2*J*B channels):
 *                                 what xsq_phasemix is without options; flags != 0
 *   xsq_wiener_em_options         niter iterations in place on Y (2*J*B channels) holding those starts (only the source count
 *                                 of flags matters here); niter = 0 leaves Y alone
 *   xsq_wiener_em_masked_options  the same fed by the MASKS (v_j = m_j |x|): Y is written only; niter = 0 with flags != 0 writes
 *                                 the starts (one elementwise launch); win_len and every S*T_b even
 *   workspace: xsq_wiener_options_workspace bytes for every niter (0 on error).  method as xsq_wiener_em_iter; the resident
 *   form holds windows of at most xsq_wiener_resident_max_window_sources(J) frames, J = 4 or 5 (0 for any other J).     */
#define XSQ_WIENER_SOFTMASK 1
#define XSQ_WIENER_RESIDUAL 2
int xsq_wiener_resident_max_window_sources(int nsources);
size_t xsq_wiener_options_workspace(int nblocks, const int32_t* F, const int32_t* T, int B, int S, int win_len, int niter,
                                    int method, int flags);
int xsq_wiener_start(int nblocks, const int32_t* F, const int32_t* T, const float* X, const float* mag, float* Y, int B, int S,
                     int flags, void* stream);
int xsq_wiener_em_options(int nblocks, const int32_t* F, const int32_t* T, const float* X, float* Y, int B, int S, int win_len,
                          int batch_group, int niter, int method, int flags, void* workspace, size_t workspace_bytes,
                          void* stream);
int xsq_wiener_em_masked_options(int nblocks, const int32_t* F, const int32_t* T, const float* X, const float* masks, float* Y,
                                 int B, int S, int win_len, int batch_group, const float* ext_max, int niter, int method,
                                 int flags, void* workspace, size_t workspace_bytes, void* stream);
/* The option set of the whole call (xsq_demix_pass, xsq_separator_*): state of the model handle, read per call.  With
 * residual set xsq_separator_forward / _indirect / _forward_segments write FIVE stems, out = (5, nb, 2, N), and size their
 * workspaces for it; xsq_separator_remix and xsq_demix_pass refuse (XSQ_ERR_ARG).  A mix-phase call (wiener = 0) with an
 * option set runs the elementwise start in place of the fused mask * X.                                              */
int xsq_model_set_wiener_options(xsq_model* model, int softmask, int residual);

/* ---- loss forward (validation half of training.loop, training.py:34-112 with train=False) -------
 * Replaces ComplexMSELossCriterion (loss.py:37-76) and MaskSumLossCriterion (loss.py:79-96).
 *   pred, target  complex arenas, 8*B channels (4 targets, B, 2, ...)
 *   masks         real arena, 8*B channels, or NULL
 *   out           DEVICE double[2*nblocks]: per block (complex-MSE mean over the 14 combinations,
 *                 mask-sum mean); the criteria average these over the blocks.
 * Any block table: the arenas are walked 16 bytes at a time where every block's real sub-arena
 * (2*B*F_b*S*T_b floats per target) is a multiple of four floats -- every table of a sliCQT plan -- and
 * the masks of EVERY block of the table 8 bytes at a time otherwise (B*F_b*S*T_b odd for some block),
 * so that every access is inside its own sub-arena and aligned to its width (an even block's mask
 * term may then differ in the last bits from what it gives in an all-even table).  The arenas themselves must be 16-byte aligned.
 * XSQ_ERR_ARG (before any device call) on a null pointer, B or S <= 0 or a workspace below
 * xsq_loss_workspace (0 on bad arguments).                                                      */
size_t xsq_loss_workspace(int nblocks, const int32_t* F, const int32_t* T, int B, int S);
int xsq_loss_forward(int nblocks, const int32_t* F, const int32_t* T, const float* pred,
                     const float* target, const float* masks, int B, int S, double* out,
                     void* workspace, size_t workspace_bytes, void* stream);

/* ---- dataset statistics (training.get_statistics, training.py:115-154) ---------------------------
 * Per block and frequency bin: sum and sum of squares over the S*T_b frames of the channel-mean
 * magnitude of X (C packed channels of ONE track).  out: DEVICE double[2 * sum_b F_b] (sum, sumsq per
 * bin, blocks back to back); the host merges tracks and forms mean / std like sklearn's
 * StandardScaler.partial_fit.  workspace >= 32 * sum_b F_b bytes.                              */
int xsq_magnitude_stats(int nblocks, const int32_t* F, const int32_t* T, const float* X, int C, int S,
                        double* out, void* workspace, size_t workspace_bytes, void* stream);

/* ---- training step (training.loop with train=True, training.py:34-112; BASELINE config 5) -------
 * One handle owns the parameters, their gradients and the AdamW moments as flat fp32 pools in the
 * xsq_model_create order (the reference's state_dict order), plus the GEMM-layout weights the
 * forward needs (re-gathered on the device every step).
 *   xsq_train_step: forward with BatchNorm on BATCH statistics (nn.BatchNorm2d.train(), running
 *   statistics updated with momentum 0.1 when apply_update != 0), loss = ComplexMSE + MaskSum
 *   (loss.py:37-96, SDR term off as in the published training), backward of every trainable tensor
 *   (what loss.backward() at training.py:107 produces), AdamW update (training.py:391-393).
 *     X        mix arena (2B channels, complex)      Yt   target arena (8B channels, complex)
 *     wiener   0: mix-phase (realtime model)         1: differentiable Wiener-EM (offline model)
 *     apply_update 0: gradients only (parameters and running statistics untouched)
 *     loss_out HOST double[2]: complex-MSE term, mask-sum term (the step waits for them,
 *              as loss.item() at training.py:110 does); NULL: do not wait, see xsq_train_loss
 *   xsq_train_read: what = 0 parameters, 1 gradients, 2 / 3 AdamW first / second moments -> HOST
 *   float[nparams].  xsq_train_write restores parameters (0) or a moment pool (2 / 3) from the host and
 *   xsq_train_step_count reads (set < 0) or restores the AdamW step counter: together they are the
 *   optimizer.state_dict() the reference checkpoints for resuming (training.py:419-430).        */
typedef struct xsq_train xsq_train;
int xsq_train_create(xsq_train** out, int nblocks, const int32_t* F, const int32_t* T, int causal,
                     const float* params, int64_t nparams);
int xsq_train_destroy(xsq_train* t);
size_t xsq_train_workspace(const xsq_train* t, int B, int S, int wiener);      /* 0 on error */
int xsq_train_step(xsq_train* t, const float* X, const float* Yt, int B, int S, int wiener,
                   float lr, float weight_decay, int apply_update, double* loss_out,
                   void* workspace, size_t workspace_bytes, void* stream);
/* loss_out == NULL: the step does not wait.  The loss terms of the last 4 steps stay retrievable by ticket
 * (xsq_train_ticket: ticket of the step issued last, 0-based count of steps on this handle); xsq_train_loss blocks
 * until that step has finished and returns its two terms -- a loop can issue step k + 1 before it looks at the loss
 * of step k, which keeps the device busy across the read-back that loss.item() makes every step.            */
int64_t xsq_train_ticket(xsq_train* t);
int xsq_train_loss(xsq_train* t, int64_t ticket, double* loss_out);
int xsq_train_read(xsq_train* t, int what, float* host_out);
int xsq_train_write(xsq_train* t, int what, const float* host_in);
int64_t xsq_train_step_count(xsq_train* t, int64_t set);
/* Arithmetic of the GEMM-shaped forward / data-gradient kernels of the step: 0 fp32 MFMA (default), 2 bf16x6 (see
 * xsq_model_set_precision), 1 = "bf16": BASELINE configs[4] as written -- the reference runs forward + loss under
 * torch.autocast(dtype=bfloat16) (training.py:66-108,473-476), i.e. its convolutions contract bf16-rounded operands.  Mode 1
 * rounds both operands of every forward, data-gradient and weight-gradient contraction to bf16 (round to nearest even) and
 * accumulates one v_mfma_f32_32x32x16_bf16 product per pair in fp32; activations between the layers, BatchNorm, the
 * Wiener-EM, the loss, the master weights and AdamW stay fp32 -- fewer rounding points than autocast, which also keeps
 * BatchNorm / ReLU / sigmoid outputs in bf16 (tests/golden/training_step_bf16.npz holds the reference's own
 * fp32-vs-autocast spread; the arm is held inside it).  The weight gradients always follow this mode (keeping them on
 * fp32 operands under mode 1 measured slower, DESIGN.md section 7, and is no longer offered).                        */
int xsq_train_set_precision(xsq_train* t, int mode);

/* ---- SDR term of the training loss (loss.py:5-34: auraloss.time.SDSDRLoss over the 14 target combinations) ----------
 * Waveforms pred / target (4, B, 2, n) on the device.  Per (b, ch) row and combination c (estimates p and targets t of
 * the members summed, both centred over the n samples):
 *   alpha = <p, t> / (<t, t> + 1e-8);   loss = -10 log10( |alpha t|^2 / (|p - t|^2 + 1e-8) + 1e-8 )
 * and the criterion is the mean over rows and combinations.  out: DEVICE double[1 + 84 B]: the criterion, then the row
 * losses it is the mean of, [b][ch][combination] (singles, pairs, triples in loss.py's order), then in the same layout the two
 * scalars A and B of every combination's gradient  scale / (28 B) * d loss_row / d p = A t + B (p - t)  (p, t centred; scale = 1 in
 * the forward call).  xsq_sdr_loss_backward also writes
 * gy (4, B, 2, n) = scale * d criterion / d pred.  Two streaming passes with fp64 moments in fixed order (no atomics); a
 * silent target gives row loss 80 and gradient 0.  XSQ_ERR_ARG on a null pointer, B or n <= 0, or a workspace below
 * xsq_sdr_loss_workspace (0 on bad arguments).                                                                        */
size_t xsq_sdr_loss_workspace(int B, int64_t n);
int xsq_sdr_loss_forward(const float* pred, const float* target, int B, int64_t n, double* out,
                         void* workspace, size_t workspace_bytes, void* stream);
int xsq_sdr_loss_backward(const float* pred, const float* target, int B, int64_t n, float scale, double* out, float* gy,
                          void* workspace, size_t workspace_bytes, void* stream);

/* ---- adjoint of the inverse sliCQT: the gradient of a time-domain loss with respect to the coefficients -------------
 * With y = xsq_slicqt_inverse(coef, BC, S, length) and gy (BC, length) = dLoss/dy, gcoef (arena of BC channels, S
 * slices) = dLoss/dcoef; accumulate != 0 adds it to what gcoef holds.  It is the analysis with a slice window of ones
 * and the window a' (xsq_slicqt_adjoint_window: host arithmetic, no device; out laid out like gd) in place of g, run
 * on the analysis kernels of the plan's back end over tables built from a' on first use (a synchronous upload).        */
int xsq_slicqt_adjoint_window(int L, int nbands, const int32_t* Lg, const int32_t* c, const double* gd, double* out);
size_t xsq_slicqt_inverse_adjoint_workspace(xsq_plan* plan, int BC, int S, int accumulate);
int xsq_slicqt_inverse_adjoint(xsq_plan* plan, const float* gy, int BC, int S, int64_t length, float* gcoef, int accumulate,
                               void* workspace, size_t workspace_bytes, void* stream);

/* ---- adjoint of the forward sliCQT: the gradient of a coefficient-domain loss with respect to the audio -------------
 * The adjoint of nsgt/slicing.py:21-72 (slices, slice window), nsgt/nsgtf.py:40-81 (FFT_L, band windows, IFFT_Lg) and
 * nsgt/slicq.py:13-33 (arrange).  With coef = xsq_slicqt_forward(x, BC, n) and gcoef (arena of BC channels,
 * S = xsq_plan_num_slices(n) slices; the real view of the coefficients' cotangent) = dLoss/dcoef, gx (BC, n) = dLoss/dx:
 *   V[s,j,q] = (-1)^(c_j/2) g_j[q] / Lg_j FFT_Lg(gcoef[s,j,:])[q],   k = (c_j + sq(q)) mod L,
 *   fr_s[k] += V (k <= L/2),  fr_s[L-k] += conj V (k > L/2),   seg_s = tw . irfft_L(w fr_s), w_0 = w_{L/2} = L, w_k = L/2,
 *   gx[m] = sum_s seg_s[m + 2h - 2sh].
 * It runs on the synthesis kernels of the plan's back end over tables built on first use (a synchronous upload) from
 * xsq_slicqt_forward_adjoint_window (host arithmetic, no device; out laid out like g: g_j[q] / Lg_j times the weight
 * w / L of the bin the entry lands on), a pass that adds the conjugates of the mirrored entries, and an overlap-add that
 * applies the slice window.  No atomics: two calls on the same input give the same bits.  XSQ_ERR_ARG on a null pointer,
 * BC or n <= 0, or a workspace below xsq_slicqt_forward_adjoint_workspace (0 on bad arguments).                         */
int xsq_slicqt_forward_adjoint_window(int L, int nbands, const int32_t* Lg, const int32_t* c, const float* g, double* out);
size_t xsq_slicqt_forward_adjoint_workspace(xsq_plan* plan, int BC, int64_t n);
int xsq_slicqt_forward_adjoint(xsq_plan* plan, const float* gcoef, int BC, int64_t n, float* gx,
                               void* workspace, size_t workspace_bytes, void* stream);

/* ---- the training step with the SDR term ---------------------------------------------------------------------------
 * xsq_train_step plus  mcoef * SDR( inverse sliCQT of the estimates, y_targets ): the estimates' inverse transform, the two
 * SDR passes and the adjoint added into the estimates' gradient run between the loss pass and the post-filter backward.
 * plan: the transform the arenas came from; y_targets (4, B, 2, n) on the device; mcoef > 0.  loss_out: HOST double[3]
 * (complex MSE, mask sum, SDR criterion unweighted); xsq_train_loss_sdr reads the same by ticket (third value 0 for a
 * step issued without the term).  The transform and SDR kernels are fp32 under every precision mode.                  */
size_t xsq_train_workspace_sdr(const xsq_train* t, xsq_plan* plan, int B, int S, int wiener, int64_t n);
int xsq_train_step_sdr(xsq_train* t, xsq_plan* plan, const float* X, const float* Yt, const float* y_targets, int64_t n,
                       float mcoef, int B, int S, int wiener, float lr, float weight_decay, int apply_update,
                       double* loss_out, void* workspace, size_t workspace_bytes, void* stream);
int xsq_train_loss_sdr(xsq_train* t, int64_t ticket, double* loss_out);

/* ---- the whole call: Separator.forward (separator.py:133-232) behind ONE entry point ----------------------------
 * The reference's chunk loop -- per chunk of <= chunk_size samples: zero-pad to sllen/2 + 1 (162-168), sliCQT (170),
 * Unmix with mix-phase or Wiener-EM (172-219), isliCQT to the chunk's length (221-227), hard concat (229-231) -- issued
 * from native code so that the host enqueues a 240 s track in ~0.1 ms instead of walking ~40 Python / ctypes calls and
 * ~300 tensor views per step (which left the eager step host-bound on slow hosts).
 *
 * xsq_demixer: per-plan cache of the row-offset tables of a call shape (device arrays, built on first use) and the
 *   fork / join events of the tail stream.  Not owned: the plan must outlive it.  The model is passed per call (its
 *   handle is rebuilt when parameters change).
 * xsq_demix_pass: ONE pass over B = items * group equal-length work items (chunks of any tracks; `group` = nb_samples
 *   of an item, the scope of the Wiener window maximum):
 *     xsq_slicqt_forward_rows (+ whitened magnitude) -> xsq_cdae_forward_xin (masks only)
 *       -> wiener == 0: xsq_slicqt_inverse_masked          (mix-phase, the estimate mask * X formed on the way in)
 *          wiener == 1: xsq_wiener_em_masked -> xsq_slicqt_inverse_rows
 *          wiener >= 2: xsq_wiener_em_masked_iter(niter = wiener, method = auto) -> xsq_slicqt_inverse_rows
 *   `wiener` is the number of EM iterations in every entry point of this section (0 and 1 keep their earlier meaning
 *   and bits; negative: XSQ_ERR_ARG).
 *   x_rows: DEVICE int64[2B] element offsets of the input rows (NULL: contiguous (B, 2, n)); out_rows: DEVICE
 *   int64[8B] element offsets of packed channel (target, item, c) in `out`; n = samples per item, n_pad as above.
 * xsq_separator_forward: audio (nb, 2, N) -> out (4, nb, 2, N), both DEVICE fp32 contiguous.  Full chunks are stacked
 *   along the batch axis, at most max_stack (chunk, sample) pairs per pass and never more rows than one launch
 *   addresses (a batch too large for one pass is split over the samples; with Wiener-EM the passes of such a set first
 *   fold their window maxima into a shared table, xsq_wiener_window_max, so the maximum keeps its batch-wide scope,
 *   norbert/__init__.py:257); the remaining chunks run one by one, on `tail_stream` beside the
 *   stacked passes when overlap_tail != 0 and tail_stream != stream (forked / joined with events: capturable in a
 *   HIP graph).  workspace / tail_workspace: xsq_separator_workspace bytes each (the tail one may be NULL when nothing
 *   runs on the tail stream).  Same bits as the chunk-by-chunk loop.  A demixer serves ONE call at a time (its fork / join
 *   events and the workspaces are per call); concurrent callers use one demixer each.                              */
typedef struct xsq_demixer xsq_demixer;
int xsq_demixer_create(xsq_demixer** out, xsq_plan* plan);
int xsq_demixer_destroy(xsq_demixer* d);
size_t xsq_demix_pass_workspace(xsq_demixer* d, const xsq_model* model, int B, int64_t n_pad, int wiener);   /* 0 on error */
int xsq_demix_pass(xsq_demixer* d, xsq_model* model, const float* x, const int64_t* x_rows, int B, int64_t n,
                   int64_t n_pad, int group, int wiener, float* out, const int64_t* out_rows,
                   void* workspace, size_t workspace_bytes, void* stream);
int xsq_separator_workspace(xsq_demixer* d, const xsq_model* model, int nb, int64_t N, int64_t chunk_size, int max_stack,
                            int wiener, size_t* main_bytes, size_t* tail_bytes);
int xsq_separator_forward(xsq_demixer* d, xsq_model* model, const float* audio, int nb, int64_t N, int64_t chunk_size,
                          int max_stack, int wiener, int overlap_tail, float* out, void* workspace,
                          size_t workspace_bytes, void* tail_workspace, size_t tail_workspace_bytes, void* stream,
                          void* tail_stream);
/* xsq_separator_forward with the audio's base pointer in a DEVICE slot (audio_slot: device address of one `const float*`),
 * read by the first kernel of every pass when it RUNS: the call can be captured once in a HIP graph and replayed on any
 * (nb, 2, N) tensor of the captured shape after an 8-byte write to the slot (Separator.forward_graphed).              */
int xsq_separator_forward_indirect(xsq_demixer* d, xsq_model* model, const float* const* audio_slot, int nb, int64_t N,
                                   int64_t chunk_size, int max_stack, int wiener, int overlap_tail, float* out,
                                   void* workspace, size_t workspace_bytes, void* tail_workspace,
                                   size_t tail_workspace_bytes, void* stream, void* tail_stream);
/* xsq_separator_forward whose result is R gain-weighted mixes of the four stems instead of the stems: out (R, nb, 2, N),
 * out[r] = sum_t gains[4 r + t] * stem_t with the targets in Separator.sources order (bass, vocals, other, drums) --
 * the slider mix of demixui.py:94-114, remix_signal of cadenza/enhance.py:270-290 and the target groups of
 * separator.py:235-259 (to_dict with aggregate_dict), through R inverse transforms per chunk instead of four
 * (xsq_slicqt_inverse_remix).  Same schedule as xsq_separator_forward: stacked full chunks, the tail chunk on
 * tail_stream, split batches with the shared Wiener window-maximum table, the sllen/2 + 1 padding.  gains: HOST
 * float[R * 4], finite, 1 <= R <= 4.  The workspaces xsq_separator_workspace returns for the call shape are enough for
 * every R <= 4; the call reads the demixer's cached row tables and changes none of them.                            */
int xsq_separator_remix(xsq_demixer* d, xsq_model* model, const float* audio, int nb, int64_t N, int64_t chunk_size,
                        int max_stack, int wiener, int overlap_tail, float* out, void* workspace, size_t workspace_bytes,
                        void* tail_workspace, size_t tail_workspace_bytes, void* stream, void* tail_stream,
                        const float* gains, int R);
/* The schedule xsq_separator_forward follows for a call shape, as pure host arithmetic (no device needed): pass i ->
 * passes[8 i ..] = (first sample of its first chunk, samples per chunk, chunks stacked, first sample index of the batch,
 * samples of the batch in this pass, 1 = may run on the tail stream, index of the first pass of its set, 1 = the set
 * shares a Wiener-EM window-maximum table).  L = slice length, coefs_per_slice = sum F_b T_b; max_item_slices <= 0: the
 * library's own cap.  Returns the number of passes (may exceed max_passes: call again), negative on error.            */
int xsq_separator_schedule(int L, int64_t coefs_per_slice, int nb_samples, int64_t N, int64_t chunk_size, int max_stack,
                           int wiener, int max_item_slices, int64_t* passes, int max_passes);
/* Test hook: cap on B * S (stacked items x slices) of one pass, normally what the 32-bit arena offsets of the band
 * kernels allow (7168); a smaller value forces the batch split on small shapes.  <= 0 restores the default.        */
int xsq_demixer_set_max_rows(xsq_demixer* d, int max_item_slices);

/* ---- overlapped, cross-faded segments: separate_sources of cadenza/enhance.py:35-99 behind ONE entry point ----------
 * The Cadenza caller of the reference does not use the hard concat of Separator.forward: it walks the track in segments
 * that overlap, fades each linearly in and out (torchaudio Fade) and adds them into the result.  The segment rule, in
 * integers: segment k = 0, 1, ... starts at (k == 0 ? 0 : k * chunk_len - ov), exists while start < N - ov and ends at
 * min((k + 1) * chunk_len, N); it fades in over its first ov samples unless k == 0 and out over its last ov samples when
 * segment k + 1 exists.  w_in[i] = i / (ov - 1), w_out[i] = 1 - i / (ov - 1) (ov == 1: 0 and 1; ov == 0: no fades).
 * Two departures from the reference text: a segment without a successor does not fade out, and the first
 * hop is chunk_len - ov in integers.
 *
 * xsq_segment_schedule: the rule as pure host arithmetic (no device needed): segs[4 i ..] = (start, samples, fade_in,
 *   fade_out) of segment i.  Returns the number of segments (may exceed max_segs: call again; 0 when N <= ov), negative
 *   on error (N < 1, chunk_len < 1, ov < 0).
 * xsq_crossfade_place: the blend of ONE pass of k equal-length segments.  scratch holds their un-faded stems as rows of n
 *   samples, packed channel (target, segment * nb + b, c) at scratch + row_offsets[...] (DEVICE int64[8 k nb], the pass's
 *   out_rows); segment j covers samples [start + j * stride, + n) of dst (4, nb, 2, N), n - stride == ov <= stride for
 *   k > 1.  Every sample of [start, start + (k - 1) * stride + n) is written once, nothing outside it:
 *     fl(fl(w_out * a) + fl(w_in * b)) where two segments of the pass meet, the plain value where the weight is 1;
 *     fade_in_first:  the first ov samples become dst + fl(w_in * b) -- the launch of the previous pass, earlier on the
 *                     same stream, stored fl(w_out * a) there (its fade_out_last) -- the same bits as the line above;
 *     fade_out_last:  the last ov samples are stored as fl(w_out * b).
 *   No atomics, no zero fill, 64-bit offsets into dst; a launch covers < 2^31 samples per row.
 * xsq_separator_forward_segments: audio (nb, 2, N) -> out (4, nb, 2, N), out[.., start_k + i] = sum_k w_k[i] *
 *   xsq_separator_forward(segment k)[.., i].  Segments of equal length (the first, the middle ones, the last) are
 *   stacked into passes of at most min(max_stack * slices of a full chunk, the demixer's cap) item-slices -- a 10 s
 *   segment has 56 slices against a full chunk's 292 -- read in place through x_rows at stride chunk_len, their stems
 *   written to scratch inside the workspace and blended into `out` by one xsq_crossfade_place launch per pass.  All passes
 *   run in segment order on `stream`.  Every (segment, sample batch) is its own Wiener item (group = nb).  `wiener` as in
 *   xsq_separator_forward.  XSQ_ERR_ARG for chunk_len + ov > chunk_size, ov >= chunk_len, ov < 0, chunk_len < 1, N <= ov
 *   and a batch whose single segment exceeds one pass (nb * slices above the cap).  Plans are cached per call shape with
 *   those of xsq_separator_forward.  workspace: xsq_separator_segments_workspace bytes.                                  */
int xsq_segment_schedule(int64_t N, int64_t chunk_len, int64_t ov, int64_t* segs, int max_segs);
int xsq_crossfade_place(const float* scratch, const int64_t* row_offsets, float* dst, int nb, int64_t N, int64_t start,
                        int64_t stride, int64_t n, int k, int ov, int fade_in_first, int fade_out_last, void* stream);
/* the same for nsources = 4 or 5 stems (the residual of xsq_model_set_wiener_options): rows (source, segment * nb + b, c) */
int xsq_crossfade_place_sources(const float* scratch, const int64_t* row_offsets, float* dst, int nsources, int nb, int64_t N,
                                int64_t start, int64_t stride, int64_t n, int k, int ov, int fade_in_first, int fade_out_last,
                                void* stream);
int xsq_separator_segments_workspace(xsq_demixer* d, const xsq_model* model, int nb, int64_t N, int64_t chunk_size,
                                     int64_t chunk_len, int64_t ov, int max_stack, int wiener, size_t* bytes);
int xsq_separator_forward_segments(xsq_demixer* d, xsq_model* model, const float* audio, int nb, int64_t N,
                                   int64_t chunk_size, int64_t chunk_len, int64_t ov, int max_stack, int wiener, float* out,
                                   void* workspace, size_t workspace_bytes, void* stream);

/* ---- the ideal-mask oracle (ideal_slicqt of xumx_slicq_v2/slicqfinder.py:43-117) -------------------------------------------
 * What a filterbank can reach at best: the true stems are transformed, their magnitudes keep the phase of the mix
 * (strategy XSQ_IDEAL_PHASEMIX) or go through one Wiener-EM iteration (XSQ_IDEAL_WIENER), and the result is inverted.
 * The forward transform of the four stems stacked as rows IS the estimates' arena (source-major, 8*B complex channels), so
 * the filters below read that arena and need neither a mix arena nor magnitudes.  Per point and channel:
 *   m   = eps + sum_j (s_j + eps) on the real and on the imaginary part, eps = 1e-10 (slicqfinder.py:57,71: 5e-10 in all);
 *   v_j = |s_j|;  start y_j = v_j m/|m| with angle(0) = 0, as xsq_phasemix.
 * xsq_phasemix_sources: Y = the starts.  xsq_wiener_em_sources: one iteration of norbert.wiener(v, m, 1, False) on them, the
 *   arithmetic of xsq_wiener_em (window statistics, the window maximum over the rows of a batch_group, the 2x2 solve per
 *   point).  Sc is read once by the statistics pass and once by the apply pass, Y is written once; Y == Sc (in place) is
 *   allowed and gives the same bits.  Both arenas 16-byte aligned.  win_len == 0: one window over all frames of a row.  One
 *   iteration only -- the entry point has no count to pass: a further one needs the mix in memory (write the estimates and call
 *   xsq_wiener_em_iter with a mix arena) -- and no softmask / residual.  No atomics: the same bits on every run.
 *   workspace: xsq_wiener_sources_workspace bytes (0 on error).
 * xsq_ideal_separate: sources (4, B, 2, n) -> estimates (4, B, 2, n), DEVICE fp32 contiguous, in one call:
 *   xsq_slicqt_forward on the 8*B rows -> the filter of `strategy` in place (batch_group = 1: every item is a track of its
 *   own) -> xsq_slicqt_inverse to n samples.  XSQ_ERR_ARG for null or misshapen arguments and for a shape whose arena does
 *   not fit one launch (xsq_ideal_workspace returns 0 for it), XSQ_ERR_WORKSPACE for a workspace below xsq_ideal_workspace. */
#define XSQ_IDEAL_WIENER 0
#define XSQ_IDEAL_PHASEMIX 1
size_t xsq_wiener_sources_workspace(int nblocks, const int32_t* F, const int32_t* T, int B, int S, int win_len);
int xsq_wiener_em_sources(int nblocks, const int32_t* F, const int32_t* T, const float* Sc, float* Y, int B, int S,
                          int win_len, int batch_group, void* workspace, size_t workspace_bytes, void* stream);
int xsq_phasemix_sources(int nblocks, const int32_t* F, const int32_t* T, const float* Sc, float* Y, int B, int S,
                         void* stream);
size_t xsq_ideal_workspace(xsq_demixer* d, int B, int64_t n, int strategy, int win_len);
int xsq_ideal_separate(xsq_demixer* d, const float* sources, int B, int64_t n, int strategy, int win_len, float* estimates,
                       void* workspace, size_t workspace_bytes, void* stream);

/* ---- the streaming session: Separator.stream, block-by-block demixing equal to one forward ---------------------------
 * With h = L / 4, slice s covers the samples [(2s - 2)h, (2s + 2)h) and block k = samples [2kh, (2k + 2)h) is the second half
 * of inverted slice k plus the first half of slice k + 1.  In mix-phase mode the mask of slice s depends on the coefficients
 * of the slices s - back .. s + XSQ_STREAM_AHEAD only (back = XSQ_STREAM_BACK_CAUSAL for the causal stack, whose first layer
 * is left-padded, XSQ_STREAM_BACK_OFFLINE for the offline one; tests/test_stream_cpu.py perturbs the oracle), so a block is
 * final 8h samples after its first one, whatever back is.  Steps fire on the ABSOLUTE block grid: step j closes the blocks
 * [j m, (j + 1) m), m = hop_slices, once sample (2 ((j + 1) m + ahead) + 2) h has been fed; what a session returns depends on
 * the samples and m only, not on how they were split into pushes.  Wiener-EM cannot stream (window statistics over 5000
 * frames from the start of a chunk): sessions are mix-phase, xsq_model_set_wiener_options must be 0.
 *
 * xsq_stream_schedule: the rule as pure host arithmetic (no device needed) for a stream of N samples in all: steps[6 j ..] =
 *   (first block, blocks, first slice inverted, first and last slice of the CDAE window, samples that must have been fed --
 *   beyond N for the steps that only the end of the stream releases).  The window is clipped to the slices N samples have
 *   (at least L / 2 + 1 samples are assumed, as the whole call pads) and never shorter than 3.  Returns the number of steps.
 * xsq_stream_create: a session of nb_samples rows on the demixer's plan (not owned).  Host state only: the DEVICE state --
 *   xsq_stream_state_bytes: an audio ring of (2 (back + ahead + m) + 2) h samples per channel, and twice the 2h-sample second
 *   half of the last inverted slice per packed output channel -- is the caller's and is passed to every call; it does not
 *   grow with the stream.  It needs no initialisation.
 * xsq_stream_push: count more samples of every row (row r at x + r * row_stride; rows (sample, channel)) into the ring, by one
 *   launch on `stream`.  XSQ_ERR_ARG when that would pass xsq_stream_next_trigger: the step has to run first.
 * xsq_stream_step: the next step, every launch on `stream`, no host synchronisation, no device-to-host read:
 *     xsq_slicqt_forward_ring (the window's slices from the ring at their absolute index; only samples before 0 and from
 *       `total` on are zero) -> xsq_cdae_forward_xin (masks of the window) -> xsq_slicqt_inverse_masked_carry (the NEW slices
 *       only: mask * mix formed on the way in, the first block added onto the carried half, the last half carried on).
 *   total < 0: the stream is open and the step's trigger must have been fed; total >= 0 (= the samples fed): the stream has
 *   ended, windows are clipped at its last slice and the last block is cut at `total`.  x / row_stride / count (count may be 0):
 *   the samples that release the step, exactly up to xsq_stream_next_trigger, instead of a push of their own -- the step's
 *   first kernel reads them where they lie and stores them to the ring.  out: packed channel (target, sample, c)
 *   at out + row * out_stride, `length` samples = what the step emits (XSQ_ERR_ARG otherwise).  workspace:
 *   xsq_stream_workspace bytes (0 on error).  A session belongs to one stream at a time.                                */
#define XSQ_STREAM_BACK_CAUSAL 3
#define XSQ_STREAM_BACK_OFFLINE 2
#define XSQ_STREAM_AHEAD 2
typedef struct xsq_stream xsq_stream;
int xsq_stream_schedule(int64_t N, int L, int hop_slices, int back, int ahead, int64_t* steps, int max_steps);
int xsq_stream_create(xsq_stream** out, xsq_demixer* d, const xsq_model* model, int nb_samples, int hop_slices, int back, int ahead);
int xsq_stream_destroy(xsq_stream* s);
size_t xsq_stream_state_bytes(const xsq_stream* s);
size_t xsq_stream_workspace(const xsq_stream* s, const xsq_model* model);
int64_t xsq_stream_next_trigger(const xsq_stream* s);
int xsq_stream_push(xsq_stream* s, void* state, const float* x, int64_t row_stride, int64_t count, void* stream);
int xsq_stream_step(xsq_stream* s, xsq_model* model, void* state, const float* x, int64_t row_stride, int64_t count, int64_t total,
                    float* out, int64_t out_stride, int64_t length, void* workspace, size_t workspace_bytes, void* stream);
/* The two transform halves of a step.  xsq_slicqt_forward_ring: S slices per channel from absolute slice first_slice on, read
 * from a ring of ring_len samples per channel that holds absolute sample i at i % ring_len; n = samples of the stream so far
 * (later ones read as zero, as do those before 0), the last new_count of which are not in the ring yet: they are read from x_new
 * (row bc at x_new + bc * new_stride) and stored to the ring; they must lie in the second halves of the call's slices.
 * xsq_slicqt_inverse_masked_carry: slices [first, first + S) of the window
 * arenas (S_window slices; masks BC channels, mix BCx) are inverted; they lie at positions shift .. of the step (shift = 0: the
 * stream's slice 0 is the first of them; 1: carry_in holds the second half of their predecessor), close S - 1 + shift blocks
 * of 2h samples, `length` samples of which are written to row bc of y (y + bc * y_stride), and leave the second half of the
 * last one in carry_out (BC x 2h floats; not carry_in).  No slice is inverted twice.                                       */
int xsq_slicqt_forward_ring(xsq_plan* plan, float* ring, int ring_len, int BC, int64_t first_slice, int S, int64_t n, const float* x_new,
                            int64_t new_stride, int64_t new_count, float* coef, float* xin, const float* mean, const float* scale,
                            int split, void* workspace, size_t workspace_bytes, void* stream);
size_t xsq_slicqt_inverse_carry_workspace(xsq_plan* plan, int BC, int BCx, int S);
int xsq_slicqt_inverse_masked_carry(xsq_plan* plan, const float* masks, const float* mix, int BC, int BCx, int S_window, int first, int S,
                                    int shift, int64_t length, float* y, int64_t y_stride, const float* carry_in, float* carry_out,
                                    void* workspace, size_t workspace_bytes, void* stream);

/* ---- scoring a separation (csrc/score.hip) -------------------------------------------------------------------------
 * Replaces the host half of evaluation.py:16-44 (museval's headline SDR) and slicqfinder.py:20-40 (_fast_sdr) for waveforms
 * that are already on the device.  A track of N samples has F = max(1, N / W) frames of W samples (hop = window); N < W is one
 * frame of N samples; a tail shorter than W belongs to no frame.  Per target i, row b and frame, over the frame's samples and
 * both channels, formed in fp64 from the fp32 samples:  num = sum s^2,  den = sum (s_hat - s)^2,  est = sum s_hat^2.
 * table (device, fp64; the CALLER zeroes it before a track's first piece): moments (4, B, F + 1, 2) = (num, den), cell F the
 *   tail, followed by the estimates' energies (4, B, F + 1), which the joint silence rule needs.
 * xsq_score_workspace: *table_bytes and *ws_bytes for a track, enough for any piece of it; refuses more than
 *   xsq_score_max_frames() frames (the median is a sort in LDS), saying so.
 * xsq_score_accumulate: adds samples [offset, offset + n) of the track to the table.  est / tgt point at the piece's first
 *   sample of row 0; row (stem j, b, channel c) lies ((j * B + b) * 2 + c) * row_stride floats further, so a view into a longer
 *   tensor is read where it lies.  Target i is row block i of tgt and row block perm[i] of est (perm: HOST array of four
 *   different values in 0..4; est holds every stem it names, a fifth, residual stem is simply never named).  16-byte loads
 *   when both strides are multiples of 4 and est and tgt share their alignment modulo 16 bytes, 4-byte loads otherwise.  Two
 *   launches; no atomics: within a launch every cell has one reduction tree and one writer, launches on one stream add in
 *   order, so one way of cutting a track into pieces gives the same bits on every run.  Pieces must not overlap.
 * xsq_score_finalise: table -> out_frames fp64 (4, B, F): 10 log10(num / den), +inf for den == 0, NaN for a silent frame
 *   (XSQ_SCORE_SILENT_ANY: some target's num or est is 0 in the frame; XSQ_SCORE_SILENT_OWN: the target's own num is 0); and
 *   out_scores fp64 (4, B, 2): the nanmedian of the frames (exact selection; the mean of the two middle values for an even
 *   count; NaN when every frame is NaN) and 10 log10((sum num + 1e-10) / (sum den + 1e-10)) over all cells, the tail included. */
#define XSQ_SCORE_SILENT_ANY 0
#define XSQ_SCORE_SILENT_OWN 1
int xsq_score_max_frames(void);
int xsq_score_workspace(int B, int64_t N, int64_t W, size_t* table_bytes, size_t* ws_bytes);
int xsq_score_accumulate(const float* est, const float* tgt, const int* perm, int B, int64_t n, int64_t est_row_stride,
                         int64_t tgt_row_stride, int64_t offset, int64_t N, int64_t W, double* table, void* ws, size_t ws_bytes,
                         void* stream);
int xsq_score_finalise(const double* table, int B, int64_t frames, int silent_mode, double* out_frames, double* out_scores,
                       void* stream);

/* ---- the sliCQT spectrogram (csrc/spectrogram.hip) ----------------------------------------------------------------------
 * The device side of visualization.py:13-35 (overlap_add_slicq) and :55-81 (blockwise_spectrogram), plus the raster that is
 * the only thing to leave the device.  Geometry as for the Wiener entry points: HOST arrays F[nblocks], T[nblocks] (T a multiple
 * of 4; at most xsq_spectrogram_max_blocks() blocks, the geometry goes to the kernels by value), S slices, hop h_b = T_b / 2;
 * no plan handle.  All pointers but F / T / N are DEVICE pointers; every launch goes to `stream`; no floating-point atomics:
 * the same input gives the same bits on every run.
 * xsq_spectrogram_overlap_add: complex arena for BC packed channels -> complex rows, block b (BC, F_b, Lout_b, 2) contiguous,
 *   blocks back to back (xsq_spectrogram_overlap_add_size floats in all, 0 on bad arguments).  flatten = 0:
 *   Lout_b = (S + 1) h_b and out[p] = 0 + x[j - 1, h_b + r] + x[j, r] for p = j h_b + r, the terms whose slice exists -- one
 *   correctly rounded fp32 add per component, the bits of the reference's loop.  flatten = 1: Lout_b = S T_b, the slices side
 *   by side.  arena and out 16-byte aligned.
 * xsq_spectrogram_db: arena for B items of two channels -> db, block b (B, F_b, N_b) fp32 contiguous, blocks back to back, in
 *   one pass: column p is overlap-add position p + h_b (h_b columns dropped at each end; flatten: position p + h_b of the
 *   slices side by side), value = mean over the two channels of 20 log10 |.| (log first, mix-down second; |.| by hypotf;
 *   |.| == 0 gives -inf and the mean of anything with -inf is -inf).  N: HOST array, 1 <= N_b <= (S - 1) h_b (flatten:
 *   S T_b - T_b), the caller's truncation min(int(T_b / L * n), ...).  S >= 2.
 * xsq_spectrogram_order_stats: for every batch item the k_lo-th and k_hi-th smallest (0-based, k_lo <= k_hi <= k_lo + 1) of
 *   ITS values in all blocks of db (sum F_b N_b < 2^32 of them; -inf counts as a value) -> out (B, 2) fp32.  Exact: a radix
 *   select over the order-preserving integer image of the floats, integer atomics only.  The quantile's lerp is the caller's.
 *   (T is not needed; one block of one row selects from a plain array.)  workspace: xsq_spectrogram_order_workspace(B) bytes.
 * xsq_spectrogram_raster: db -> image (B, sum F_b, W) fp32, row = band; row f of block b, column w = max of that row's
 *   columns [lo, hi), lo = w N_b / W, hi = max(lo + 1, (w + 1) N_b / W) in 64-bit integers. */
int xsq_spectrogram_max_blocks(void);
int64_t xsq_spectrogram_overlap_add_size(int nblocks, const int32_t* F, const int32_t* T, int BC, int S, int flatten);
int xsq_spectrogram_overlap_add(int nblocks, const int32_t* F, const int32_t* T, const float* arena, int BC, int S, int flatten,
                                float* out, void* stream);
int xsq_spectrogram_db(int nblocks, const int32_t* F, const int32_t* T, const int32_t* N, const float* arena, int B, int S,
                       int flatten, float* db, void* stream);
size_t xsq_spectrogram_order_workspace(int B);
int xsq_spectrogram_order_stats(int nblocks, const int32_t* F, const int32_t* N, const float* db, int B, int64_t k_lo, int64_t k_hi,
                                float* out, void* workspace, size_t workspace_bytes, void* stream);
int xsq_spectrogram_raster(int nblocks, const int32_t* F, const int32_t* N, const float* db, int B, int W, float* image,
                           void* stream);

/* ---- per-kernel timing (bench.py roofline) ------------------------------------------
 * When enabled, every kernel launch of the library is bracketed by hipEvents recorded on
 * its own launch stream.  xsq_profile_read synchronises the outstanding events and
 * returns accumulated milliseconds / launch counts per kernel name (newline-separated
 * names, same order as ms[] / launches[]); returns the number of entries.              */
int xsq_profile_enable(int on);
int xsq_profile_reset(void);
/* Time only the kernel launched under this event name (NULL or "": all kernels).  Two event records around every
 * launch cost ~0.1 ms per 24-launch step; bench.py times every kernel in its warm-up steps and only the dominant
 * one inside the timed region.                                                                              */
int xsq_profile_filter(const char* name);
int xsq_profile_read(char* names, size_t names_bytes, double* ms, int64_t* launches,
                     int max_entries);

#ifdef __cplusplus
}
#endif
#endif /* XUMX_SLICQ_HIP_H */
