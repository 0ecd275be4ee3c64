"""ctypes binding of the C ABI in include/xumx_slicq_hip.h.

The HIP library is the product: there is NO CPU fallback.  Importing this
module without the built library raises immediately with build instructions,
and every call checks its status code and raises ``XsqError`` with the
library's message.
"""
from __future__ import annotations

import ctypes as C
import os

import torch  # noqa: F401  (must come first: it loads the ROCm runtime this library binds to)

_HERE = os.path.dirname(os.path.abspath(__file__))
# XSQ_LIB selects a diagnostic build (tools/ablate.sh); the default is the product library.
LIB_PATH = os.environ.get("XSQ_LIB") or os.path.join(_HERE, "libxumx_slicq_hip.so")


class XsqError(RuntimeError):
    pass


def _load():
    if not os.path.exists(LIB_PATH):
        raise XsqError(
            f"{LIB_PATH} is missing: the HIP extension is the product path and has no CPU "
            "fallback. Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C xumx_slicq_amd/csrc`.")
    # torch has already mapped its own libamdhip64.so / librocfft.so (same SONAMEs as the
    # system ROCm ones this library was linked against), so the loader resolves our
    # NEEDED entries to the copies torch uses and both sides share one HIP runtime.
    return C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)


lib = _load()

_vp = C.c_void_p
_i32p = C.POINTER(C.c_int32)
_i64p = C.POINTER(C.c_int64)

_SIGS = {
    "xsq_abi_version": (C.c_int, []),
    "xsq_last_error": (C.c_char_p, []),
    "xsq_build_info": (C.c_char_p, []),
    "xsq_plan_create": (C.c_int, [C.POINTER(_vp), C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp]),
    "xsq_plan_create_twins": (C.c_int, [C.POINTER(_vp), C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp]),
    "xsq_plan_num_twins": (C.c_int, [_vp]),
    "xsq_plan_create_flags": (C.c_int, [C.POINTER(_vp), C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, C.c_uint]),
    "xsq_plan_long_band_max": (C.c_int, []),
    "xsq_plan_long_band_min": (C.c_int, []),
    "xsq_plan_num_long_bands": (C.c_int, [_vp]),
    "xsq_plan_destroy": (C.c_int, [_vp]),
    "xsq_plan_num_blocks": (C.c_int, [_vp]),
    "xsq_plan_set_fft_backend": (C.c_int, [_vp, C.c_int]),
    "xsq_plan_set_band_radix4": (C.c_int, [_vp, C.c_int]),
    "xsq_plan_set_short_inline": (C.c_int, [_vp, C.c_int]),
    "xsq_plan_set_packed_fft": (C.c_int, [_vp, C.c_int]),
    "xsq_plan_block_table": (C.c_int, [_vp, _vp]),
    "xsq_plan_coefs_per_slice": (C.c_int64, [_vp]),
    "xsq_plan_num_slices": (C.c_int, [_vp, C.c_int64]),
    "xsq_slicqt_forward_workspace": (C.c_size_t, [_vp, C.c_int, C.c_int64]),
    "xsq_slicqt_forward": (C.c_int, [_vp, _vp, C.c_int, C.c_int64, _vp, _vp, C.c_size_t, _vp]),
    "xsq_slicqt_forward_xin": (C.c_int, [_vp, _vp, C.c_int, C.c_int64, _vp, _vp, _vp, _vp, C.c_int, _vp, C.c_size_t, _vp]),
    "xsq_slicqt_forward_rows": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int64, C.c_int64, _vp, _vp, _vp, _vp, C.c_int, _vp, C.c_size_t, _vp]),
    "xsq_slicqt_forward_rows_indirect": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int, C.c_int64, C.c_int64, _vp, _vp, _vp, _vp, C.c_int, _vp, C.c_size_t, _vp]),
    "xsq_slicqt_inverse_workspace": (C.c_size_t, [_vp, C.c_int, C.c_int]),
    "xsq_slicqt_inverse": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int64, _vp, _vp, C.c_size_t, _vp]),
    "xsq_slicqt_inverse_rows": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int64, _vp, _vp, _vp, C.c_size_t, _vp]),
    "xsq_slicqt_inverse_masked": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int64, _vp, _vp, _vp, C.c_size_t, _vp]),
    "xsq_slicqt_remix_workspace": (C.c_size_t, [_vp, C.c_int, C.c_int, C.c_int, C.c_int]),
    "xsq_slicqt_inverse_remix": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int64, _vp, _vp, _vp, C.c_size_t, _vp]),
    "xsq_model_num_params": (C.c_int64, [C.c_int, _vp, _vp]),
    "xsq_model_create": (C.c_int, [C.POINTER(_vp), C.c_int, _vp, _vp, C.c_int, _vp, C.c_int64]),
    "xsq_model_destroy": (C.c_int, [_vp]),
    "xsq_model_set_precision": (C.c_int, [_vp, C.c_int]),
    "xsq_model_set_winograd": (C.c_int, [_vp, C.c_int]),
    "xsq_cdae_workspace": (C.c_size_t, [_vp, C.c_int, C.c_int]),
    "xsq_cdae_forward": (C.c_int, [_vp, _vp, C.c_int, C.c_int, _vp, _vp, _vp, C.c_size_t, _vp]),
    "xsq_cdae_forward_xin": (C.c_int, [_vp, _vp, C.c_int, C.c_int, _vp, _vp, _vp, C.c_size_t, _vp, C.c_int]),
    "xsq_model_whitening": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(C.c_int)]),
    "xsq_phasemix": (C.c_int, [C.c_int, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, _vp]),
    "xsq_wiener_workspace": (C.c_size_t, [C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int]),
    "xsq_loss_workspace": (C.c_size_t, [C.c_int, _vp, _vp, C.c_int, C.c_int]),
    "xsq_loss_forward": (C.c_int, [C.c_int, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, _vp, _vp, C.c_size_t, _vp]),
    "xsq_magnitude_stats": (C.c_int, [C.c_int, _vp, _vp, _vp, C.c_int, C.c_int, _vp, _vp, C.c_size_t, _vp]),
    "xsq_train_create": (C.c_int, [C.POINTER(_vp), C.c_int, _vp, _vp, C.c_int, _vp, C.c_int64]),
    "xsq_train_destroy": (C.c_int, [_vp]),
    "xsq_train_workspace": (C.c_size_t, [_vp, C.c_int, C.c_int, C.c_int]),
    "xsq_train_step": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, _vp, _vp, C.c_size_t, _vp]),
    "xsq_train_ticket": (C.c_int64, [_vp]),
    "xsq_train_loss": (C.c_int, [_vp, C.c_int64, _vp]),
    "xsq_train_read": (C.c_int, [_vp, C.c_int, _vp]),
    "xsq_train_write": (C.c_int, [_vp, C.c_int, _vp]),
    "xsq_train_step_count": (C.c_int64, [_vp, C.c_int64]),
    "xsq_train_set_precision": (C.c_int, [_vp, C.c_int]),
    "xsq_sdr_loss_workspace": (C.c_size_t, [C.c_int, C.c_int64]),
    "xsq_sdr_loss_forward": (C.c_int, [_vp, _vp, C.c_int, C.c_int64, _vp, _vp, C.c_size_t, _vp]),
    "xsq_sdr_loss_backward": (C.c_int, [_vp, _vp, C.c_int, C.c_int64, C.c_float, _vp, _vp, _vp, C.c_size_t, _vp]),
    "xsq_slicqt_adjoint_window": (C.c_int, [C.c_int, C.c_int, _vp, _vp, _vp, _vp]),
    "xsq_slicqt_dropped_twin_share": (C.c_int, [C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp]),
    "xsq_slicqt_inverse_adjoint_workspace": (C.c_size_t, [_vp, C.c_int, C.c_int, C.c_int]),
    "xsq_slicqt_inverse_adjoint": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int64, _vp, C.c_int, _vp, C.c_size_t, _vp]),
    "xsq_slicqt_forward_adjoint_window": (C.c_int, [C.c_int, C.c_int, _vp, _vp, _vp, _vp]),
    "xsq_slicqt_forward_adjoint_workspace": (C.c_size_t, [_vp, C.c_int, C.c_int64]),
    "xsq_slicqt_forward_adjoint": (C.c_int, [_vp, _vp, C.c_int, C.c_int64, _vp, _vp, C.c_size_t, _vp]),
    "xsq_train_workspace_sdr": (C.c_size_t, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int64]),
    "xsq_train_step_sdr": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int64, C.c_float, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int,
                                     _vp, _vp, C.c_size_t, _vp]),
    "xsq_train_loss_sdr": (C.c_int, [_vp, C.c_int64, _vp]),
    "xsq_place_rows": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int64, _vp]),
    "xsq_resample": (C.c_int, [_vp, C.c_int64, C.c_int, C.c_int64, _vp, C.c_int64, C.c_int64, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp]),
    "xsq_wiener_num_windows": (C.c_int64, [C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int]),
    "xsq_wiener_window_max": (C.c_int, [C.c_int, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp]),
    "xsq_wiener_em_masked_ext": (C.c_int, [C.c_int, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_size_t, _vp]),
    "xsq_demixer_create": (C.c_int, [C.POINTER(_vp), _vp]),
    "xsq_demixer_destroy": (C.c_int, [_vp]),
    "xsq_demixer_set_max_rows": (C.c_int, [_vp, C.c_int]),
    "xsq_separator_schedule": (C.c_int, [C.c_int, C.c_int64, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, _vp, C.c_int]),
    "xsq_demix_pass_workspace": (C.c_size_t, [_vp, _vp, C.c_int, C.c_int64, C.c_int]),
    "xsq_demix_pass": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int, _vp, _vp, _vp, C.c_size_t, _vp]),
    "xsq_separator_workspace": (C.c_int, [_vp, _vp, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "xsq_separator_forward": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_size_t, _vp, C.c_size_t, _vp, _vp]),
    "xsq_separator_forward_indirect": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_size_t, _vp, C.c_size_t, _vp, _vp]),
    "xsq_separator_remix": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_size_t, _vp, C.c_size_t, _vp, _vp, _vp, C.c_int]),
    "xsq_segment_schedule": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, _vp, C.c_int]),
    "xsq_crossfade_place": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, _vp]),
    "xsq_separator_segments_workspace": (C.c_int, [_vp, _vp, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    "xsq_separator_forward_segments": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int, _vp, _vp, C.c_size_t, _vp]),
    "xsq_stream_schedule": (C.c_int, [C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.c_int]),
    "xsq_stream_create": (C.c_int, [C.POINTER(_vp), _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int]),
    "xsq_stream_destroy": (C.c_int, [_vp]),
    "xsq_stream_state_bytes": (C.c_size_t, [_vp]),
    "xsq_stream_workspace": (C.c_size_t, [_vp, _vp]),
    "xsq_stream_next_trigger": (C.c_int64, [_vp]),
    "xsq_stream_push": (C.c_int, [_vp, _vp, _vp, C.c_int64, C.c_int64, _vp]),
    "xsq_stream_step": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int64, C.c_int64, C.c_int64, _vp, C.c_int64, C.c_int64, _vp, C.c_size_t, _vp]),
    "xsq_slicqt_forward_ring": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int64, _vp, C.c_int64, C.c_int64, _vp, _vp, _vp, _vp, C.c_int,
                                          _vp, C.c_size_t, _vp]),
    "xsq_slicqt_inverse_carry_workspace": (C.c_size_t, [_vp, C.c_int, C.c_int, C.c_int]),
    "xsq_slicqt_inverse_masked_carry": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, _vp, C.c_int64, _vp, _vp,
                                                  _vp, C.c_size_t, _vp]),
    "xsq_comm_load": (C.c_int, [C.c_char_p]),
    "xsq_comm_version": (C.c_int, []),
    "xsq_comm_unique_id": (C.c_int, [_vp]),
    "xsq_comm_create": (C.c_int, [C.POINTER(_vp), _vp, C.c_int, C.c_int]),
    "xsq_comm_destroy": (C.c_int, [_vp]),
    "xsq_comm_abort": (C.c_int, [_vp]),
    "xsq_exchange_rows": (C.c_int, [_vp, _vp, C.c_int64, _vp, C.c_int64, _vp, C.c_int, C.c_int, _vp]),
    "xsq_profile_enable": (C.c_int, [C.c_int]),
    "xsq_profile_reset": (C.c_int, []),
    "xsq_profile_filter": (C.c_int, [C.c_char_p]),
    "xsq_profile_read": (C.c_int, [C.c_char_p, C.c_size_t, _vp, _vp, C.c_int]),
    "xsq_wiener_em": (C.c_int, [C.c_int, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.c_size_t, _vp]),
    "xsq_wiener_em_masked": (C.c_int, [C.c_int, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.c_size_t, _vp]),
    "xsq_wiener_resident_max_window": (C.c_int, []),
    "xsq_wiener_iter_workspace": (C.c_size_t, [C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "xsq_wiener_em_iter": (C.c_int, [C.c_int, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.c_size_t, _vp]),
    "xsq_wiener_em_masked_iter": (C.c_int, [C.c_int, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.c_int, C.c_int, _vp,
                                            C.c_size_t, _vp]),
    "xsq_wiener_resident_max_window_sources": (C.c_int, [C.c_int]),
    "xsq_wiener_options_workspace": (C.c_size_t, [C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "xsq_wiener_start": (C.c_int, [C.c_int, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp]),
    "xsq_wiener_em_options": (C.c_int, [C.c_int, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.c_size_t,
                                        _vp]),
    "xsq_wiener_em_masked_options": (C.c_int, [C.c_int, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.c_int, C.c_int, C.c_int,
                                               _vp, C.c_size_t, _vp]),
    "xsq_model_set_wiener_options": (C.c_int, [_vp, C.c_int, C.c_int]),
    "xsq_crossfade_place_sources": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int,
                                              C.c_int, _vp]),
    "xsq_batch_assemble": (C.c_int, [_vp, C.c_int, _vp, C.c_int, _vp, C.c_int64, C.c_int, C.c_int64, _vp, _vp, _vp, _vp]),
    "xsq_score_max_frames": (C.c_int, []),
    "xsq_score_workspace": (C.c_int, [C.c_int, C.c_int64, C.c_int64, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "xsq_score_accumulate": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, _vp, _vp,
                                       C.c_size_t, _vp]),
    "xsq_score_finalise": (C.c_int, [_vp, C.c_int, C.c_int64, C.c_int, _vp, _vp, _vp]),
    "xsq_wiener_sources_workspace": (C.c_size_t, [C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int]),
    "xsq_wiener_em_sources": (C.c_int, [C.c_int, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.c_size_t, _vp]),
    "xsq_phasemix_sources": (C.c_int, [C.c_int, _vp, _vp, _vp, _vp, C.c_int, C.c_int, _vp]),
    "xsq_ideal_workspace": (C.c_size_t, [_vp, C.c_int, C.c_int64, C.c_int, C.c_int]),
    "xsq_ideal_separate": (C.c_int, [_vp, _vp, C.c_int, C.c_int64, C.c_int, C.c_int, _vp, _vp, C.c_size_t, _vp]),
    "xsq_spectrogram_max_blocks": (C.c_int, []),
    "xsq_spectrogram_overlap_add_size": (C.c_int64, [C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int]),
    "xsq_spectrogram_overlap_add": (C.c_int, [C.c_int, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp]),
    "xsq_spectrogram_db": (C.c_int, [C.c_int, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp]),
    "xsq_spectrogram_order_workspace": (C.c_size_t, [C.c_int]),
    "xsq_spectrogram_order_stats": (C.c_int, [C.c_int, _vp, _vp, _vp, C.c_int, C.c_int64, C.c_int64, _vp, _vp, C.c_size_t, _vp]),
    "xsq_spectrogram_raster": (C.c_int, [C.c_int, _vp, _vp, _vp, C.c_int, C.c_int, _vp, _vp]),
}

for _name, (_res, _args) in _SIGS.items():
    _fn = getattr(lib, _name)
    _fn.restype = _res
    _fn.argtypes = _args

EXPORTED = tuple(_SIGS)
PLAN_TWINS, PLAN_LONG_BANDS = 1, 2       # the flags of xsq_plan_create_flags: XSQ_PLAN_TWINS, XSQ_PLAN_LONG_BANDS (include/xumx_slicq_hip.h)


def build_info() -> dict:
    """What is loaded: path, ABI version, the library's own build string (xsq_build_info)."""
    return {"path": LIB_PATH, "default_path": LIB_PATH == os.path.join(_HERE, "libxumx_slicq_hip.so"),
            "abi": int(lib.xsq_abi_version()), "build": (lib.xsq_build_info() or b"").decode("utf-8", "replace")}


def xsq_environment() -> dict:
    """Every XSQ_* variable set in this process: most of them select kernels, fusions or diagnostic paths (csrc getenv,
    separator.py / model.py / transforms.py switches).  bench.py records them and flags a line measured with any."""
    return {k: v for k, v in sorted(os.environ.items()) if k.startswith("XSQ_")}


def last_error() -> str:
    return (lib.xsq_last_error() or b"").decode("utf-8", "replace")


def check(rc: int, what: str):
    if rc != 0:
        raise XsqError(f"{what} failed ({rc}): {last_error()}")


def call(name: str, *args):
    """The native entry point ``name`` on ``args``; ``XsqError`` naming it, with the library's message, unless it returns 0."""
    check(getattr(lib, name)(*args), name)


def workspace_bytes(name: str, *args, why=None) -> int:
    """Bytes the size query ``name`` asks for.  A query refuses with 0: ``XsqError`` naming it.  ``why`` is the reason where the
    query sets no error text of its own -- the library's buffer is per thread and never cleared, so it may hold the message of
    an earlier call."""
    nbytes = getattr(lib, name)(*args)
    if nbytes == 0:
        raise XsqError(f"{name}: {why or last_error()}")
    return nbytes


def stream_ptr() -> int:
    """The HIP stream torch is currently issuing work on."""
    return torch.cuda.current_stream().cuda_stream


def device_index(device) -> int:
    """The index of a ROCm ``torch.device``; one without an index is torch's current device."""
    return device.index if device.index is not None else torch.cuda.current_device()


class Scratch(dict):
    """Grow-only workspaces of one owner: {(device index, stream pointer, tag): uint8 tensor}.  Calls issued on different
    streams may overlap, so every stream has its own buffer.  PyTorch owns the memory.

    Captured graphs hold raw pointers into these buffers, so a buffer stays where it is while it is large enough and is
    never replaced by a smaller one; whoever captures keeps ``tensors()`` alive with the graph.  A copy or pickle of a pool
    is an empty pool: the copy allocates its own on first use."""

    FLOOR = 256     # what a zero-byte request gets: the alignment unit of the library's workspace layouts

    def get(self, device, nbytes: int, stream=None, tag=None):
        """At least ``nbytes`` bytes on ``device`` for work on ``stream`` (a stream pointer; default: torch's current stream of
        that device); ``tag`` tells apart the buffers one owner uses side by side on one stream."""
        key = (device_index(device), torch.cuda.current_stream(device).cuda_stream if stream is None else stream, tag)
        ws = dict.get(self, key)
        if ws is None or ws.numel() < nbytes:
            ws = self[key] = None               # drop the old buffer first: the allocator may hand its pages to the new one
            ws = self[key] = self._allocate(int(nbytes) or self.FLOOR, device)
        return ws

    @staticmethod
    def _allocate(nbytes: int, device):
        return torch.empty(nbytes, dtype=torch.uint8, device=device)

    def tensors(self) -> list:
        return [ws for ws in self.values() if ws is not None]

    def __deepcopy__(self, memo):
        return type(self)()

    def __reduce__(self):
        return type(self), ()


def profile_enable(on: bool = True):
    lib.xsq_profile_enable(1 if on else 0)


def profile_reset():
    lib.xsq_profile_reset()


def profile_filter(name=None):
    """Time only the kernel launched under this event name (None: all kernels)."""
    lib.xsq_profile_filter(name.encode() if name else None)


def profile_read() -> dict:
    """{kernel name: (total ms, launches)} accumulated since the last reset."""
    import numpy as np
    buf = C.create_string_buffer(8192)
    ms = np.zeros(128, dtype=np.float64)
    cnt = np.zeros(128, dtype=np.int64)
    n = lib.xsq_profile_read(buf, len(buf), ms.ctypes.data, cnt.ctypes.data, 128)
    names = buf.value.decode().split("\n")[:n]
    return {nm: (float(ms[i]), int(cnt[i])) for i, nm in enumerate(names)}
