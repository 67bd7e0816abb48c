"""ctypes bindings for libmfcchip.so and the Python mirror of the reference's parameterizer API.

``MfccHip`` keeps the method names, argument meaning and error behaviour of the reference's
``ParamBase`` / ``MfccBase`` interface (parambase.h:6-33, mfccbase.h:21-35) that ``MfccCpu`` and
``MfccOpenCL`` implement: ``set_window, set_input, flush, set_alpha, apply,
get_output_data_width, get_output_data, get_input_buffer_size, estimated_window_count``.
Errors the reference throws as ``std::runtime_error`` surface as ``MfxError`` with the same text.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))

NORM_NONE, NORM_CMN, NORM_CVN, NORM_MINMAX = 0, 1, 2, 3   # normalizer.h:5
DYN_NONE, DYN_DELTA, DYN_ACC = 0, 1, 2                     # parambase.h:9
METHOD_MFCC, METHOD_PLP = 0, 1                             # mfx_config.method (include/mfx.h)
METHOD_TRAPS = 3                                           # (2 is unassigned and refused)
METHOD_STFT_LOGMEL = 5                                     # (4 is unassigned and refused)
METHOD_KALDI = 7                                           # (6 is unassigned and refused)
LOGMEL_WHISPER, LOGMEL_LOG10, LOGMEL_LN = 0, 1, 2          # mfx_config.logmel_post (include/mfx.h)
KALDI_NO_SNIP_EDGES, KALDI_USE_ENERGY, KALDI_ENERGY_WINDOWED, KALDI_HTK_COMPAT = 1, 2, 4, 8   # kaldi_flags of mfx_create_kaldi


class MfxError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(message)
        self.status = status


class MfxConfig(C.Structure):
    """POD mirror of ``mfx_config`` (include/mfx.h)."""
    _fields_ = [
        ("input_buffer_size", C.c_int32),
        ("window_size", C.c_int32),
        ("shift", C.c_int32),
        ("num_banks", C.c_int32),
        ("sample_rate", C.c_float),
        ("low_freq", C.c_float),
        ("high_freq", C.c_float),
        ("ceps_len", C.c_int32),
        ("want_c0", C.c_int32),
        ("lift_coef", C.c_float),
        ("norm", C.c_int32),
        ("dyn", C.c_int32),
        ("delta_l1", C.c_int32),
        ("delta_l2", C.c_int32),
        ("norm_after_dyn", C.c_int32),
        ("fft_size", C.c_int32),
        ("channels", C.c_int32),
        ("bug_compat", C.c_int32),
        ("batch_norm_stats", C.c_int32),
        ("engine", C.c_int32),
        ("tail_split", C.c_int32),
        ("method", C.c_int32),
        ("lpc_order", C.c_int32),
        ("traps_len", C.c_int32),
        ("traps_dct_len", C.c_int32),
        ("logmel_post", C.c_int32),
    ]


# every symbol include/mfx.h declares
EXPORTED_SYMBOLS = (
    "mfx_create", "mfx_destroy", "mfx_last_error", "mfx_status_string", "mfx_abi_version",
    "mfx_set_window", "mfx_set_input", "mfx_flush", "mfx_set_alpha", "mfx_apply",
    "mfx_get_output_data_width", "mfx_get_output_data", "mfx_get_input_buffer_size",
    "mfx_apply_alphas", "mfx_get_output_data_alpha", "mfx_host_mel_lane_plan",
    "mfx_host_dct_mfma_operands",
    "mfx_estimated_window_count", "mfx_max_frames_out", "mfx_fft_size",
    "mfx_batch_frames", "mfx_batch_plan", "mfx_batch_run_device", "mfx_batch_run_host", "mfx_batch_overlap",
    "mfx_batch_set_alphas", "mfx_host_alpha_runs",
    "mfx_batch_set_transform", "mfx_batch_output_width", "mfx_host_xform_operands",
    "mfx_alloc_pinned", "mfx_free_pinned",
    "mfx_set_stream", "mfx_synchronize", "mfx_profile_enable", "mfx_profile_read",
    "mfx_dominant_kernel_name", "mfx_debug_read", "mfx_plan_create", "mfx_plan_set_aligned",
    "mfx_host_mel_table", "mfx_host_dct_matrix", "mfx_host_frame_count",
    "mfx_method_supported", "mfx_host_plp_tables", "mfx_host_traps_basis",
    "mfx_sessions_create", "mfx_sessions_reset", "mfx_sessions_plan", "mfx_sessions_run_device", "mfx_sessions_run_host",
    "mfx_sessions_delivered", "mfx_host_session_step",
    "mfx_sessions_set_transform", "mfx_sessions_clear_transform", "mfx_sessions_select_transform",
    "mfx_sessions_output_width", "mfx_host_session_xform_step", "mfx_host_sess_xform_groups",
    "mfx_sessions_set_rates", "mfx_sessions_clear_rates", "mfx_sessions_select_rate", "mfx_sessions_converted_read",
    "mfx_host_session_resample_step",
    "mfx_batch_plan_rates", "mfx_batch_resample_layout", "mfx_host_resample_taps", "mfx_host_resampled_length",
    "mfx_host_resample_layout", "mfx_host_resample_tile",
    "mfx_batch_set_speakers", "mfx_batch_speaker_stats", "mfx_host_speaker_lists",
    "mfx_batch_set_vad", "mfx_batch_clear_vad", "mfx_batch_vad_read", "mfx_batch_vad_device",
    "mfx_batch_set_online_norm", "mfx_batch_clear_online_norm", "mfx_sessions_set_online_norm",
    "mfx_sessions_clear_online_norm", "mfx_host_online_norm",
    "mfx_batch_set_sliding_norm", "mfx_batch_clear_sliding_norm", "mfx_host_sliding_window", "mfx_host_sliding_norm",
    "mfx_host_slaney_mel_table", "mfx_host_stft_basis", "mfx_host_stft_frame_count",
    "mfx_host_stft_lds_bytes", "mfx_host_session_stft_step", "mfx_host_sess_stft_lds_bytes",
    "mfx_host_stft_fft_tables", "mfx_host_stft_fft_lds_bytes",
    "mfx_kaldi_set_options", "mfx_host_kaldi_mel_table", "mfx_host_kaldi_dct", "mfx_host_kaldi_lds_bytes",
    "mfx_create_kaldi", "mfx_plan_create_kaldi", "mfx_kaldi_flags_supported", "mfx_host_kaldi_lds_bytes_flags", "mfx_host_kaldi_frame_count", "mfx_host_kaldi_frame_samples",
    "mfx_batch_set_pitch", "mfx_batch_clear_pitch", "mfx_batch_pitch_read", "mfx_batch_pitch_device", "mfx_host_pitch",
    "mfx_batch_set_pitch_feats", "mfx_batch_clear_pitch_feats", "mfx_batch_pitch_feats_read", "mfx_batch_pitch_feats_device",
    "mfx_host_pitch_feats",
    "mfx_batch_set_tensor", "mfx_batch_clear_tensor", "mfx_batch_output_bytes", "mfx_batch_tensor_shape",
    "mfx_batch_tensor_lengths", "mfx_batch_tensor_from_rows",
    "mfx_host_tensor_pack", "mfx_host_tensor_bytes", "mfx_host_tensor_lds_bytes",
    "mfx_batch_fuse_info", "mfx_host_delta_tile_lds_floats", "mfx_host_fuse_claim",
)


def library_path():
    # MFX_LIB: developer override to A/B an experimental build of the same ABI
    return os.environ.get("MFX_LIB") or os.path.join(_HERE, "libmfcchip.so")


_lib = None


def load_library():
    """Load libmfcchip.so and declare the prototypes.  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    p = library_path()
    if not os.path.exists(p):
        raise MfxError(-6, "libmfcchip.so is not built (run __graft_entry__.build()); there is no CPU fallback")
    # PyTorch-ROCm wheels bundle their own libamdhip64/libhsa-runtime64.  A process must hold ONE HIP
    # runtime: if torch is going to be used alongside (device tensors, torch.distributed), it has to be
    # loaded first so that libmfcchip.so binds to the runtime already in the process instead of
    # bringing /opt/rocm's in as a second one ("no ROCm-capable device" on whichever comes second).
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    L = C.CDLL(p)
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    fp, sp = C.POINTER(C.c_float), C.POINTER(C.c_int16)
    L.mfx_create.argtypes = [C.POINTER(MfxConfig), C.c_int, C.POINTER(vp)]
    L.mfx_destroy.argtypes = [vp]
    L.mfx_destroy.restype = None
    L.mfx_last_error.argtypes, L.mfx_last_error.restype = [vp], C.c_char_p
    L.mfx_status_string.argtypes, L.mfx_status_string.restype = [C.c_int], C.c_char_p
    L.mfx_abi_version.argtypes = []
    L.mfx_set_window.argtypes = [vp, fp]
    L.mfx_set_input.argtypes = [vp, sp, i32, C.POINTER(i32)]
    L.mfx_flush.argtypes = [vp, C.POINTER(i32)]
    L.mfx_set_alpha.argtypes = [vp, C.c_float]
    L.mfx_apply.argtypes = [vp]
    L.mfx_get_output_data_width.argtypes = [vp]
    L.mfx_get_output_data.argtypes = [vp, fp, i32]
    L.mfx_apply_alphas.argtypes = [vp, fp, i32]
    L.mfx_get_output_data_alpha.argtypes = [vp, i32, fp, i32]
    L.mfx_get_input_buffer_size.argtypes = [vp]
    L.mfx_estimated_window_count.argtypes = [vp, i32]
    L.mfx_max_frames_out.argtypes = [vp]
    L.mfx_fft_size.argtypes = [vp]
    L.mfx_batch_frames.argtypes, L.mfx_batch_frames.restype = [vp, i64], i64
    L.mfx_batch_plan.argtypes = [vp, i32, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)]
    L.mfx_batch_run_device.argtypes = [vp, vp, i64, vp]
    L.mfx_batch_run_host.argtypes = [vp, sp, i64, fp]
    L.mfx_batch_overlap.argtypes = [vp, C.c_int]
    L.mfx_batch_set_alphas.argtypes = [vp, fp, i32]
    L.mfx_host_alpha_runs.argtypes = [i32, fp, C.POINTER(i64), i64, i64, fp, C.POINTER(i32), C.POINTER(i64)]
    L.mfx_host_alpha_runs.restype = i64
    L.mfx_batch_set_transform.argtypes = [vp, i32, i32, i32, i32, fp, fp, C.POINTER(i32), i32]
    L.mfx_batch_output_width.argtypes = [vp]
    L.mfx_host_xform_operands.argtypes = [i32, i32, fp, fp, i64, C.POINTER(i32), C.POINTER(i32)]
    L.mfx_host_xform_operands.restype = i64
    L.mfx_set_stream.argtypes = [vp, vp]
    L.mfx_synchronize.argtypes = [vp]
    L.mfx_profile_enable.argtypes = [vp, C.c_int]
    L.mfx_profile_read.argtypes = [vp, C.POINTER(i32), C.POINTER(C.c_double), C.c_int]
    L.mfx_dominant_kernel_name.argtypes, L.mfx_dominant_kernel_name.restype = [vp], C.c_char_p
    L.mfx_plan_create.argtypes = [C.POINTER(MfxConfig), C.POINTER(vp)]
    L.mfx_batch_fuse_info.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)]
    L.mfx_host_delta_tile_lds_floats.argtypes, L.mfx_host_delta_tile_lds_floats.restype = [i32, i32, i32, C.POINTER(i32)], i32
    L.mfx_host_fuse_claim.argtypes, L.mfx_host_fuse_claim.restype = [i64, i32, C.POINTER(i32)], i64
    L.mfx_plan_set_aligned.argtypes = [vp, C.c_int]
    L.mfx_debug_read.argtypes, L.mfx_debug_read.restype = [vp, C.c_int, vp, i64], i64
    L.mfx_host_mel_table.argtypes = [i32, i32, C.c_float, C.c_float, C.c_float, C.c_float, fp, C.POINTER(i32)]
    L.mfx_host_dct_matrix.argtypes = [i32, i32, i32, C.c_float, fp]
    L.mfx_host_frame_count.argtypes, L.mfx_host_frame_count.restype = [i64, i32, i32], i64
    L.mfx_method_supported.argtypes = [i32]
    L.mfx_host_plp_tables.argtypes = [i32, i32, C.c_float, C.c_float, C.c_float, C.c_float, i32, fp, fp]
    L.mfx_host_traps_basis.argtypes = [i32, i32, fp]
    p32, p64 = C.POINTER(i32), C.POINTER(i64)
    L.mfx_sessions_create.argtypes = [vp, i32, i32]
    L.mfx_sessions_reset.argtypes = [vp, i32]
    L.mfx_sessions_plan.argtypes = [vp, i32, p32, p64, p64, p32, p64, p32, p64]
    L.mfx_sessions_run_device.argtypes = [vp, vp, i64, vp]
    L.mfx_sessions_run_host.argtypes = [vp, sp, i64, fp]
    L.mfx_sessions_delivered.argtypes, L.mfx_sessions_delivered.restype = [vp, i32], i64
    L.mfx_host_session_step.argtypes = [i32, i32, i32, p64, i64, i32, p64, p32, p32, p32]
    L.mfx_host_session_step.restype = i32
    L.mfx_sessions_set_transform.argtypes = [vp, i32, i32, i32, i32, fp, fp]
    L.mfx_sessions_clear_transform.argtypes = [vp]
    L.mfx_sessions_select_transform.argtypes = [vp, i32, i32]
    L.mfx_sessions_output_width.argtypes = [vp]
    L.mfx_host_session_xform_step.argtypes = [i32, i32, p64, i32, i32, p32, p32]
    L.mfx_host_session_xform_step.restype = i32
    L.mfx_sessions_set_rates.argtypes = [vp, i32, p32, i32, C.c_float]
    L.mfx_sessions_clear_rates.argtypes = [vp]
    L.mfx_sessions_select_rate.argtypes = [vp, i32, i32]
    L.mfx_sessions_converted_read.argtypes, L.mfx_sessions_converted_read.restype = [vp, sp, i64, p64, p64], i64
    L.mfx_host_session_resample_step.argtypes = [i32, i32, i32, C.c_float, p64, i64, i32, p32, p32]
    L.mfx_host_session_resample_step.restype = i64
    L.mfx_host_sess_xform_groups.argtypes = [i32, p32, p32, i32, p32, i32, p32, i32, p32]
    L.mfx_host_sess_xform_groups.restype = i32
    L.mfx_batch_plan_rates.argtypes = [vp, i32, p64, p64, p32, i32, C.c_float, p64, p64]
    L.mfx_batch_resample_layout.argtypes = [vp, p64, p64, p64]
    L.mfx_host_resample_taps.argtypes = [i32, i32, i32, C.c_float, fp, i64, p32, p32, p32]
    L.mfx_host_resample_taps.restype = i64
    L.mfx_host_resampled_length.argtypes, L.mfx_host_resampled_length.restype = [i64, i32, i32], i64
    L.mfx_host_resample_layout.argtypes, L.mfx_host_resample_layout.restype = [i32, p64, p32, i32, p64, p64], i64
    L.mfx_host_resample_tile.argtypes, L.mfx_host_resample_tile.restype = [i32, i32, i32, C.c_float, i32], i32
    dp = C.POINTER(C.c_double)
    L.mfx_batch_set_speakers.argtypes = [vp, p32, i32, i32, p64, dp, i32]
    L.mfx_batch_speaker_stats.argtypes = [vp, p64, dp, fp]
    L.mfx_host_speaker_lists.argtypes, L.mfx_host_speaker_lists.restype = [i32, p32, p64, i32, p32, p32], i64
    L.mfx_batch_set_vad.argtypes = [vp, i32, C.c_float, C.c_float, i32, C.c_float, i32]
    L.mfx_batch_clear_vad.argtypes = [vp]
    L.mfx_batch_vad_read.argtypes = [vp, C.POINTER(C.c_uint8), p32, fp, p64]
    L.mfx_batch_vad_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    L.mfx_batch_set_online_norm.argtypes = [vp, i32, i32, i64, dp]
    L.mfx_batch_clear_online_norm.argtypes = [vp]
    L.mfx_sessions_set_online_norm.argtypes = [vp, i32, i32, i64, dp]
    L.mfx_sessions_clear_online_norm.argtypes = [vp]
    L.mfx_host_online_norm.argtypes = [fp, i64, i32, i32, i32, i32, i32, i64, dp, fp]
    L.mfx_batch_set_sliding_norm.argtypes = [vp, i32, i32, i32, i32]
    L.mfx_batch_clear_sliding_norm.argtypes = [vp]
    L.mfx_host_sliding_window.argtypes = [i64, i32, i32, i32, i64, C.POINTER(i64), C.POINTER(i64)]
    L.mfx_host_sliding_norm.argtypes = [fp, i64, i32, i32, i32, i32, i32, i32, fp, i32]
    L.mfx_host_slaney_mel_table.argtypes = [i32, i32, C.c_float, C.c_float, C.c_float, fp, p32, p32]
    L.mfx_host_stft_basis.argtypes = [i32, fp, fp]
    L.mfx_host_stft_frame_count.argtypes, L.mfx_host_stft_frame_count.restype = [i64, i32, i32], i64
    L.mfx_host_stft_lds_bytes.argtypes, L.mfx_host_stft_lds_bytes.restype = [i32, i32, i32, p32], i64
    L.mfx_host_stft_fft_tables.argtypes = [i32, fp, fp]
    L.mfx_host_stft_fft_lds_bytes.argtypes, L.mfx_host_stft_fft_lds_bytes.restype = [i32, i32, i32, p32], i64
    L.mfx_host_session_stft_step.argtypes, L.mfx_host_session_stft_step.restype = [i32, i32, p64, i64, i32, p32, p32], i32
    L.mfx_host_sess_stft_lds_bytes.argtypes, L.mfx_host_sess_stft_lds_bytes.restype = [i32, i32, i32, p32], i64
    L.mfx_kaldi_set_options.argtypes = [vp, C.c_float, i32, i32]
    L.mfx_host_kaldi_mel_table.argtypes = [i32, i32, C.c_float, C.c_float, C.c_float, fp, p32, p32]
    L.mfx_host_kaldi_dct.argtypes = [i32, i32, C.c_float, fp]
    L.mfx_host_kaldi_lds_bytes.argtypes, L.mfx_host_kaldi_lds_bytes.restype = [i32, i32, i32, i32], i64
    L.mfx_kaldi_flags_supported.argtypes, L.mfx_kaldi_flags_supported.restype = [], i32
    L.mfx_create_kaldi.argtypes = [C.POINTER(MfxConfig), i32, C.c_float, C.c_int, C.POINTER(vp)]
    L.mfx_plan_create_kaldi.argtypes = [C.POINTER(MfxConfig), i32, C.c_float, C.POINTER(vp)]
    L.mfx_host_kaldi_lds_bytes_flags.argtypes, L.mfx_host_kaldi_lds_bytes_flags.restype = [i32, i32, i32, i32, i32], i64
    L.mfx_host_kaldi_frame_count.argtypes, L.mfx_host_kaldi_frame_count.restype = [i64, i32, i32, i32], i64
    L.mfx_host_kaldi_frame_samples.argtypes = [i64, i32, i32, i32, i64, C.POINTER(C.c_int64)]
    L.mfx_batch_set_pitch.argtypes = [vp, i32, i32, i32, C.c_float, C.c_float, C.c_float, i32]
    L.mfx_batch_clear_pitch.argtypes = [vp]
    L.mfx_batch_pitch_read.argtypes = [vp, fp, p32, fp]
    L.mfx_batch_pitch_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    L.mfx_host_pitch.argtypes = [sp, i64, i32, i64, i32, i32, i32, i32, C.c_float, C.c_float, C.c_float, i32, fp, p32, fp]
    L.mfx_batch_set_pitch_feats.argtypes = [vp, i32, i32, i32, i32, C.c_float, C.c_float, C.c_float, C.c_float, i32]
    L.mfx_batch_clear_pitch_feats.argtypes = [vp]
    L.mfx_batch_pitch_feats_read.argtypes = [vp, fp]
    L.mfx_batch_pitch_feats_device.argtypes = [vp, C.POINTER(vp), p32]
    L.mfx_host_pitch_feats.argtypes = [fp, i64, C.c_float, i32, i32, i32, i32, C.c_float, C.c_float, C.c_float, C.c_float, fp]
    L.mfx_batch_set_tensor.argtypes = [vp, i32, i32, i32, C.c_float]
    L.mfx_batch_clear_tensor.argtypes = [vp]
    L.mfx_batch_output_bytes.argtypes, L.mfx_batch_output_bytes.restype = [vp], i64
    L.mfx_batch_tensor_shape.argtypes = [vp, C.POINTER(i64), C.POINTER(i32)]
    L.mfx_batch_tensor_lengths.argtypes = [vp, C.POINTER(i32), C.POINTER(vp)]
    L.mfx_batch_tensor_from_rows.argtypes = [vp, vp, vp]
    L.mfx_host_tensor_pack.argtypes = [fp, C.POINTER(i64), C.POINTER(i32), i64, i32, i64, i32, i32, C.c_float, vp]
    L.mfx_host_tensor_bytes.argtypes, L.mfx_host_tensor_bytes.restype = [i64, i32, i64, i32], i64
    L.mfx_host_tensor_lds_bytes.argtypes, L.mfx_host_tensor_lds_bytes.restype = [i32, C.POINTER(i32)], i64
    _lib = L
    return L


def host_mel_table(num_banks, fft_size, sample_rate, low_freq, high_freq, alpha=1.0):
    """Mel table exactly as uploaded to the device (host code, no GPU needed)."""
    L = load_library()
    w = np.zeros((2, fft_size), dtype=np.float32)
    beg = np.zeros(num_banks + 2, dtype=np.int32)
    rc = L.mfx_host_mel_table(num_banks, fft_size, sample_rate, low_freq, high_freq, alpha,
                              w.ctypes.data_as(C.POINTER(C.c_float)), beg.ctypes.data_as(C.POINTER(C.c_int32)))
    if rc != 0:
        raise MfxError(rc, "mfx_host_mel_table failed")
    return w, beg


def host_mel_lane_plan(lanes, weights, beg, max_read_bin):
    """Lane plan of the fused kernels' mel walk (lanes = 16, 32 or 64): dict(rounds, L, row_stride, start, fid, w)."""
    L = load_library()
    weights = np.ascontiguousarray(weights, dtype=np.float32)
    beg = np.ascontiguousarray(beg, dtype=np.int32)
    nb, fft = beg.size - 2, weights.shape[1]
    ip, fpt = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    fn = L.mfx_host_mel_lane_plan
    fn.argtypes = [C.c_int32, C.c_int32, C.c_int32, fpt, ip, C.c_int32, ip, ip, ip, ip, fpt, C.c_int64]
    fn.restype = C.c_int
    Ls = np.zeros(8, np.int32)
    rs = C.c_int32(0)
    rounds = fn(lanes, nb, fft, weights.ctypes.data_as(fpt), beg.ctypes.data_as(ip), int(max_read_bin),
                Ls.ctypes.data_as(ip), C.byref(rs), None, None, None, 0)
    if rounds < 0:
        raise MfxError(rounds, "mfx_host_mel_lane_plan failed")
    start = np.zeros((rounds, lanes), np.int32)
    fid = np.zeros((rounds, lanes), np.int32)
    w = np.zeros((lanes, rs.value), np.float32)
    rc = fn(lanes, nb, fft, weights.ctypes.data_as(fpt), beg.ctypes.data_as(ip), int(max_read_bin), Ls.ctypes.data_as(ip),
            C.byref(rs), start.ctypes.data_as(ip), fid.ctypes.data_as(ip), w.ctypes.data_as(fpt), w.size)
    if rc != rounds:
        raise MfxError(rc, "mfx_host_mel_lane_plan failed")
    return dict(rounds=rounds, L=Ls[:rounds].copy(), row_stride=rs.value, start=start, fid=fid, w=w)


def host_dct_mfma_operands(matrix):
    """[tile][K step][64] operands of the DCT on the matrix pipe for a [num_banks][dct_len] matrix."""
    L = load_library()
    m = np.ascontiguousarray(matrix, dtype=np.float32)
    nb, dl = m.shape
    fpt = C.POINTER(C.c_float)
    fn = L.mfx_host_dct_mfma_operands
    fn.argtypes = [C.c_int32, C.c_int32, fpt, fpt, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    fn.restype = C.c_int64
    tl, ks = C.c_int32(0), C.c_int32(0)
    n = fn(nb, dl, m.ctypes.data_as(fpt), None, 0, C.byref(tl), C.byref(ks))
    out = np.zeros(n, np.float32)
    fn(nb, dl, m.ctypes.data_as(fpt), out.ctypes.data_as(fpt), out.size, C.byref(tl), C.byref(ks))
    return out.reshape(tl.value, ks.value, 64)


def host_dct_matrix(num_banks, ceps_len, want_c0, lift_coef):
    L = load_library()
    m = np.zeros((num_banks, ceps_len + (1 if want_c0 else 0)), dtype=np.float32)
    rc = L.mfx_host_dct_matrix(num_banks, ceps_len, int(bool(want_c0)), lift_coef,
                               m.ctypes.data_as(C.POINTER(C.c_float)))
    if rc != 0:
        raise MfxError(rc, "mfx_host_dct_matrix failed")
    return m


def method_supported(method):
    """True when the loaded library computes feature method `method` (METHOD_*)."""
    return bool(load_library().mfx_method_supported(int(method)))


def _check_method(method):
    # a library older than mfx_config.method ignores the field and would quietly return MFCC
    if int(method) != METHOD_MFCC and not method_supported(method):
        raise MfxError(-5, "feature method %d is not supported by %s" % (int(method), library_path()))


def host_plp_tables(num_banks, fft_size, sample_rate, low_freq, high_freq, alpha=1.0, lpc_order=8):
    """PLP tables exactly as uploaded (host code, no GPU needed): equal-loudness weights [num_banks] and the
    autocorrelation basis [lpc_order + 1][num_banks + 2]."""
    L = load_library()
    eql = np.zeros(num_banks, dtype=np.float32)
    idft = np.zeros((lpc_order + 1, num_banks + 2), dtype=np.float32)
    fpt = C.POINTER(C.c_float)
    rc = L.mfx_host_plp_tables(int(num_banks), int(fft_size), float(sample_rate), float(low_freq), float(high_freq),
                               float(alpha), int(lpc_order), eql.ctypes.data_as(fpt), idft.ctypes.data_as(fpt))
    if rc != 0:
        raise MfxError(rc, "mfx_host_plp_tables failed")
    return eql, idft


def host_traps_basis(traps_len, traps_dct_len):
    """TRAPS basis exactly as uploaded (host code, no GPU needed): [traps_dct_len][traps_len], Hamming window times DCT-II."""
    L = load_library()
    b = np.zeros((int(traps_dct_len), int(traps_len)), dtype=np.float32)
    rc = L.mfx_host_traps_basis(int(traps_len), int(traps_dct_len), b.ctypes.data_as(C.POINTER(C.c_float)))
    if rc != 0:
        raise MfxError(rc, "mfx_host_traps_basis failed")
    return b


def host_alpha_runs(alphas, frames, window=None):
    """Run lists of mfx_batch_set_alphas exactly as uploaded (host code, no GPU needed): (tables, off, runs) for one warp
    factor and one frame count per utterance; runs is [n][2] = (first row, rows).  window = (row0, rows) clips every run
    as the kernels clip it to a slab."""
    L = load_library()
    a = np.ascontiguousarray(alphas, dtype=np.float32)
    f = np.ascontiguousarray(frames, dtype=np.int64)
    assert a.size == f.size
    n = int(a.size)
    tables = np.zeros(max(n, 1), np.float32)
    off = np.zeros(n + 1, np.int32)
    runs = np.zeros((max(n, 1), 2), np.int64)
    w0, wn = (0, -1) if window is None else (int(window[0]), int(window[1]))
    nt = L.mfx_host_alpha_runs(n, a.ctypes.data_as(C.POINTER(C.c_float)), f.ctypes.data_as(C.POINTER(C.c_int64)), w0, wn,
                               tables.ctypes.data_as(C.POINTER(C.c_float)), off.ctypes.data_as(C.POINTER(C.c_int32)),
                               runs.ctypes.data_as(C.POINTER(C.c_int64)))
    if nt < 0:
        raise MfxError(int(nt), "mfx_host_alpha_runs failed")
    nt = int(nt)
    return tables[:nt].copy(), off[:nt + 1].copy(), runs[:int(off[nt])].copy()


def host_speaker_lists(utt_spk, frames, n_spk=None):
    """Speaker lists of batch_set_speakers exactly as uploaded (host code, no GPU needed): (off [n_spk + 1], list) -- speaker
    s owns list[off[s]:off[s + 1]], its utterances in ascending order, frameless utterances left out."""
    L = load_library()
    ids = np.ascontiguousarray(utt_spk, dtype=np.int32)
    f = np.ascontiguousarray(frames, dtype=np.int64)
    assert ids.size == f.size
    if n_spk is None:
        n_spk = int(ids.max()) + 1 if ids.size else 0
    off = np.zeros(int(n_spk) + 1, np.int32)
    lst = np.zeros(max(ids.size, 1), np.int32)
    p32 = C.POINTER(C.c_int32)
    n = L.mfx_host_speaker_lists(int(ids.size), ids.ctypes.data_as(p32), f.ctypes.data_as(C.POINTER(C.c_int64)), int(n_spk),
                                 off.ctypes.data_as(p32), lst.ctypes.data_as(p32))
    if n < 0:
        raise MfxError(int(n), "mfx_host_speaker_lists failed")
    return off, lst[:int(n)].copy()


def host_online_norm(rows, kind, window=0, prior_frames=0, prior_count=0, prior_acc=None, wn=None):
    """The online normaliser of batch_set_online_norm on host memory, exactly as include/mfx.h defines it (host code, no GPU
    needed): rows [T][pitch] float32, the first wn columns (None: all) -> [T][wn].  kind: 1 CMN, 2 CVN; prior_acc [2][wn]."""
    L = load_library()
    x = np.ascontiguousarray(rows, dtype=np.float32)
    if x.ndim != 2:
        raise ValueError("rows must be [T][pitch]")
    T, pitch = x.shape
    wn = pitch if wn is None else int(wn)
    pa = None if prior_acc is None else np.ascontiguousarray(prior_acc, dtype=np.float64)
    if pa is not None and pa.size != 2 * wn:
        raise ValueError("prior_acc must be [2][wn]")
    out = np.zeros((T, max(wn, 0)), np.float32)
    fpt = C.POINTER(C.c_float)
    rc = L.mfx_host_online_norm(x.ctypes.data_as(fpt), T, pitch, wn, int(kind), int(window), int(prior_frames), int(prior_count),
                                None if pa is None else pa.ctypes.data_as(C.POINTER(C.c_double)), out.ctypes.data_as(fpt))
    if rc != 0:
        raise MfxError(int(rc), "mfx_host_online_norm failed")
    return out


def host_sliding_window(T, window, min_window, center, t):
    """The window [ws, we) of row t of an utterance of T rows under batch_set_sliding_norm (host code, no GPU needed)."""
    ws, we = C.c_int64(0), C.c_int64(0)
    rc = load_library().mfx_host_sliding_window(int(T), int(window), int(min_window), int(center), int(t), C.byref(ws), C.byref(we))
    if rc != 0:
        raise MfxError(int(rc), "mfx_host_sliding_window failed")
    return ws.value, we.value


def host_sliding_norm(rows, window=600, min_window=100, center=False, norm_vars=False):
    """The sliding-window normaliser of batch_set_sliding_norm on host memory, exactly as include/mfx.h defines it (host code,
    no GPU needed): rows [T][W] float32 -> [T][W]."""
    x = np.ascontiguousarray(rows, dtype=np.float32)
    if x.ndim != 2:
        raise ValueError("rows must be [T][W]")
    T, W = x.shape
    out = np.zeros((T, W), np.float32)
    fpt = C.POINTER(C.c_float)
    rc = load_library().mfx_host_sliding_norm(x.ctypes.data_as(fpt), T, W, W, int(window), int(min_window), int(center), int(norm_vars),
                                              out.ctypes.data_as(fpt), W)
    if rc != 0:
        raise MfxError(int(rc), "mfx_host_sliding_norm failed")
    return out


TENSOR_TIME_MAJOR, TENSOR_CHANNEL_MAJOR = 0, 1            # mfx_batch_set_tensor layouts (include/mfx.h)
DTYPE_F32, DTYPE_F16, DTYPE_BF16 = 0, 1, 2                 # ... and element types
_TENSOR_NP = {DTYPE_F32: np.float32, DTYPE_F16: np.float16, DTYPE_BF16: np.uint16}   # (numpy has no bfloat16: its bits)


def host_tensor_bytes(B, Wo, Tp, dtype):
    """Bytes of the tensor of batch_set_tensor: B * Tp * Wo elements of dtype (host code, no GPU needed)."""
    n = int(load_library().mfx_host_tensor_bytes(int(B), int(Wo), int(Tp), int(dtype)))
    if n < 0:
        raise MfxError(n, "mfx_host_tensor_bytes failed")
    return n


def host_tensor_tile():
    """(rows t per block of k_tensor_pack, a function Wo -> the LDS bytes of a CHANNEL_MAJOR block).  UNSTABLE: tests only."""
    L = load_library()
    r = C.c_int32(0)
    L.mfx_host_tensor_lds_bytes(1, C.byref(r))
    return int(r.value), (lambda Wo: int(L.mfx_host_tensor_lds_bytes(int(Wo), None)))


def host_tensor_pack(rows, out_rows, lengths, Tp, layout, dtype, pad=0.0):
    """The tensor of batch_set_tensor on host memory, exactly as include/mfx.h defines it, conversions in integer arithmetic
    (host code, no GPU needed): rows [.][Wo] float32, utterance u's from row out_rows[u] on, lengths[u] of them counting (cut
    at Tp).  Returns [B][Tp][Wo] (TENSOR_TIME_MAJOR) or [B][Wo][Tp] as float32 / float16 / uint16 (the bits of bfloat16)."""
    L = load_library()
    x = np.ascontiguousarray(rows, dtype=np.float32)
    if x.ndim != 2:
        raise ValueError("rows must be [.][Wo]")
    Wo = x.shape[1]
    r0 = np.ascontiguousarray(out_rows, dtype=np.int64)
    ln = np.ascontiguousarray(lengths, dtype=np.int32)
    B, Tp = int(r0.size), int(Tp)
    if ln.size != B or int(dtype) not in _TENSOR_NP:
        raise ValueError("one length per utterance, dtype one of DTYPE_*")
    out = np.zeros((B, Tp, Wo) if int(layout) == TENSOR_TIME_MAJOR else (B, Wo, Tp), _TENSOR_NP[int(dtype)])
    rc = L.mfx_host_tensor_pack(x.ctypes.data_as(C.POINTER(C.c_float)), r0.ctypes.data_as(C.POINTER(C.c_int64)),
                                ln.ctypes.data_as(C.POINTER(C.c_int32)), B, Wo, Tp, int(layout), int(dtype), float(pad),
                                C.c_void_p(out.ctypes.data))
    if rc != 0:
        raise MfxError(int(rc), "mfx_host_tensor_pack failed")
    return out


def host_pitch(pcm, frames, shift, window, lag_min, lag_max, ballast=0.0, lag_cost=0.0, penalty=0.0, max_jump=0, channels=1):
    """The pitch track of batch_set_pitch on host memory, exactly as include/mfx.h defines it (host code, no GPU needed), for
    one utterance: pcm int16 (interleaved for channels = 2), frames = its frame count on the handle in question.  Returns
    (lag [T], rho [T], index [T], nccf [T][K])."""
    L = load_library()
    x = np.ascontiguousarray(pcm, dtype=np.int16).reshape(-1)
    n, T, K = x.size // max(int(channels), 1), max(int(frames), 0), max(int(lag_max) - int(lag_min) + 1, 0)
    pitch, index, nccf = np.zeros((T, 2), np.float32), np.zeros(T, np.int32), np.zeros((T, min(K, 512)), np.float32)
    fpt = C.POINTER(C.c_float)
    rc = L.mfx_host_pitch(x.ctypes.data_as(C.POINTER(C.c_int16)), n, int(channels), int(frames), int(shift), int(window), int(lag_min),
                          int(lag_max), float(ballast), float(lag_cost), float(penalty), int(max_jump), pitch.ctypes.data_as(fpt),
                          index.ctypes.data_as(C.POINTER(C.c_int32)), nccf.ctypes.data_as(fpt))
    if rc != 0:
        raise MfxError(int(rc), "mfx_host_pitch failed")
    return pitch[:, 0].copy(), pitch[:, 1].copy(), index, nccf


def _pf_count(columns):
    c = int(columns)
    return bin(c if c else 7).count("1") if 0 <= c <= 15 else 0


def host_pitch_feats(lag, rho, sample_rate, columns=0, left=75, right=75, delta_window=2, pov_scale=2.0, pov_offset=0.0,
                     pitch_scale=2.0, delta_scale=10.0):
    """The pitch features of batch_set_pitch_feats on host memory, as include/mfx.h defines them (host code, no GPU needed),
    for one utterance: lag [T], rho [T] as batch_pitch_read / host_pitch return them.  Returns feats [T][F] float32."""
    L = load_library()
    pitch = np.ascontiguousarray(np.stack((np.asarray(lag, np.float32).reshape(-1), np.asarray(rho, np.float32).reshape(-1)), axis=1))
    T = pitch.shape[0]
    out = np.zeros((T, _pf_count(columns)), np.float32)
    fpt = C.POINTER(C.c_float)
    rc = L.mfx_host_pitch_feats(pitch.ctypes.data_as(fpt), T, float(sample_rate), int(columns), int(left), int(right),
                                int(delta_window), float(pov_scale), float(pov_offset), float(pitch_scale), float(delta_scale),
                                out.ctypes.data_as(fpt))
    if rc != 0:
        raise MfxError(int(rc), "mfx_host_pitch_feats failed")
    return out


def host_xform_operands(A):
    """One transform of batch_set_transform exactly as k_splice_affine streams it (host code, no GPU needed):
    [steps][tiles][64] for a matrix A [out_dim][in_dim]; element [s][t][lane] = A[16 t + (lane & 15)][4 s + (lane >> 4)]."""
    L = load_library()
    a = np.ascontiguousarray(A, dtype=np.float32)
    od, ind = a.shape
    fpt = C.POINTER(C.c_float)
    tl, st = C.c_int32(0), C.c_int32(0)
    n = L.mfx_host_xform_operands(od, ind, a.ctypes.data_as(fpt), None, 0, C.byref(tl), C.byref(st))
    if n < 0:
        raise MfxError(int(n), "mfx_host_xform_operands failed")
    out = np.zeros(n, np.float32)
    L.mfx_host_xform_operands(od, ind, a.ctypes.data_as(fpt), out.ctypes.data_as(fpt), out.size, C.byref(tl), C.byref(st))
    return out.reshape(st.value, tl.value, 64)


def host_session_step(window_size, shift, D, state, length, final=False):
    """One push of one session exactly as the planner of the session entries derives it (host code, no GPU needed).
    state = (n, E): samples received and rows delivered so far.  Returns dict(rows, state, carry_samples, carry_rows,
    new_frames, n_out, shift, lo, hi, static_off); state is (0, 0) after a final push."""
    L = load_library()
    st = (C.c_int64 * 2)(int(state[0]), int(state[1]))
    cs, cr, nf = C.c_int64(0), C.c_int32(0), C.c_int32(0)
    seg = (C.c_int32 * 5)()
    rows = L.mfx_host_session_step(int(window_size), int(shift), int(D), st, int(length), int(bool(final)), C.byref(cs),
                                   C.byref(cr), C.byref(nf), seg)
    if rows < 0:
        raise MfxError(int(rows), "mfx_host_session_step failed")
    return dict(rows=int(rows), state=(int(st[0]), int(st[1])), carry_samples=cs.value, carry_rows=cr.value,
                new_frames=nf.value, n_out=seg[0], shift=seg[1], lo=seg[2], hi=seg[3], static_off=seg[4])


def host_session_xform_step(left, right, state, n_y, final=False):
    """One push of one session under a session transform exactly as the planner derives it (host code, no GPU needed).
    state = (Ey, Ex): finished rows y and transformed rows delivered so far; n_y: the rows y the push completes.  Returns
    dict(rows, state, carry_rows, src_row0, lo, hi); state is (0, 0) after a final push."""
    L = load_library()
    st = (C.c_int64 * 2)(int(state[0]), int(state[1]))
    cr = C.c_int32(0)
    win = (C.c_int32 * 3)()
    rows = L.mfx_host_session_xform_step(int(left), int(right), st, int(n_y), int(bool(final)), C.byref(cr), win)
    if rows < 0:
        raise MfxError(int(rows), "mfx_host_session_xform_step failed")
    return dict(rows=int(rows), state=(int(st[0]), int(st[1])), carry_rows=cr.value, src_row0=win[0], lo=win[1], hi=win[2])


def host_session_resample_step(in_hz, out_hz, state, length, final=False, zeros=0, rolloff=0.0):
    """One push of one session under a session rate exactly as the planner derives it (host code, no GPU needed).  state =
    (N_in, J): input samples received and converted samples held so far.  Returns dict(n_out, state, carry_in, carry_out);
    state is (0, 0) after a final push."""
    L = load_library()
    st = (C.c_int64 * 2)(int(state[0]), int(state[1]))
    ci, co = C.c_int32(0), C.c_int32(0)
    n = L.mfx_host_session_resample_step(int(in_hz), int(out_hz), int(zeros), float(rolloff), st, int(length), int(bool(final)),
                                         C.byref(ci), C.byref(co))
    if n < 0:
        raise MfxError(int(n), "mfx_host_session_resample_step failed")
    return dict(n_out=int(n), state=(int(st[0]), int(st[1])), carry_in=ci.value, carry_out=co.value)


def host_session_stft_step(dft_size, shift, state, length, final=False):
    """One push of one session of an STFT log-mel handle exactly as the planner derives it (host code, no GPU needed).  state
    = (n, E): samples received and rows delivered so far.  Returns dict(rows, state, carry_in, carry_out); state is (0, 0)
    after a final push."""
    L = load_library()
    st = (C.c_int64 * 2)(int(state[0]), int(state[1]))
    ci, co = C.c_int32(0), C.c_int32(0)
    rows = L.mfx_host_session_stft_step(int(dft_size), int(shift), st, int(length), int(bool(final)), C.byref(ci), C.byref(co))
    if rows < 0:
        raise MfxError(int(rows), "mfx_host_session_stft_step failed")
    return dict(rows=int(rows), state=(int(st[0]), int(st[1])), carry_in=ci.value, carry_out=co.value)


def host_sess_stft_lds_bytes(dft_size, shift, num_banks, groups=0):
    """(LDS bytes of a block of k_sess_stft_mel, groups per block): at the packing mfx_sessions_create takes (groups=0), or at
    1, 2 or 4 groups per block.  UNSTABLE inspection aid."""
    L = load_library()
    g = C.c_int32(int(groups))
    n = L.mfx_host_sess_stft_lds_bytes(int(dft_size), int(shift), int(num_banks), C.byref(g))
    if n < 0:
        raise MfxError(int(n), "mfx_host_sess_stft_lds_bytes failed")
    return int(n), g.value


def host_sess_xform_groups(n_out, xf, G=4):
    """The work list of k_sess_xform (UNSTABLE inspection aid): (groups [.][3] = piece, first row, rows; blocks [.][3] = first
    group, groups, transform)."""
    L = load_library()
    no = np.ascontiguousarray(n_out, dtype=np.int32)
    x = np.ascontiguousarray(xf, dtype=np.int32)
    assert no.size == x.size
    p32 = C.POINTER(C.c_int32)
    nb = C.c_int32(0)
    ng = L.mfx_host_sess_xform_groups(no.size, no.ctypes.data_as(p32), x.ctypes.data_as(p32), int(G), None, 0, None, 0, C.byref(nb))
    if ng < 0:
        raise MfxError(int(ng), "mfx_host_sess_xform_groups failed")
    groups, blocks = np.zeros((ng, 3), np.int32), np.zeros((nb.value, 3), np.int32)
    L.mfx_host_sess_xform_groups(no.size, no.ctypes.data_as(p32), x.ctypes.data_as(p32), int(G), groups.ctypes.data_as(p32), ng,
                                 blocks.ctypes.data_as(p32), nb.value, C.byref(nb))
    return groups, blocks


def host_resample_taps(in_hz, out_hz, zeros=0, rolloff=0.0):
    """Tap table of the sample-rate converter exactly as uploaded (host code, no GPU needed): (taps [L][P], L, M, P)."""
    lib = load_library()
    L, M, P = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    n = lib.mfx_host_resample_taps(int(in_hz), int(out_hz), int(zeros), float(rolloff), None, 0, C.byref(L), C.byref(M), C.byref(P))
    if n < 0:
        raise MfxError(int(n), "mfx_host_resample_taps: shape outside the limits")
    taps = np.zeros(int(n), np.float32)
    lib.mfx_host_resample_taps(int(in_hz), int(out_hz), int(zeros), float(rolloff), taps.ctypes.data_as(C.POINTER(C.c_float)),
                               taps.size, C.byref(L), C.byref(M), C.byref(P))
    return taps.reshape(L.value, P.value), L.value, M.value, P.value


def host_resampled_length(samples, in_hz, out_hz):
    """ceil(samples * L / M): samples per channel after conversion."""
    n = int(load_library().mfx_host_resampled_length(int(samples), int(in_hz), int(out_hz)))
    if n < 0:
        raise MfxError(n, "mfx_host_resampled_length failed")
    return n


def host_resample_layout(lengths, rates, out_hz):
    """Layout of the converted PCM (host code, no GPU needed): (offsets, out_lengths, total) in output-rate samples per
    channel for utterances of the given input lengths and rates."""
    ln = np.ascontiguousarray(lengths, dtype=np.int64)
    rt = np.ascontiguousarray(rates, dtype=np.int32)
    assert ln.size == rt.size
    off, out = np.zeros(ln.size, np.int64), np.zeros(ln.size, np.int64)
    p64 = C.POINTER(C.c_int64)
    total = load_library().mfx_host_resample_layout(ln.size, ln.ctypes.data_as(p64), rt.ctypes.data_as(C.POINTER(C.c_int32)),
                                                    int(out_hz), off.ctypes.data_as(p64), out.ctypes.data_as(p64))
    if total < 0:
        raise MfxError(int(total), "mfx_host_resample_layout failed")
    return off, out, int(total)


def host_resample_tile(in_hz, out_hz, zeros=0, rolloff=0.0, channels=1):
    """Output samples per tile of k_resample for a rate pair (test aid: utterance lengths at a tile edge)."""
    n = int(load_library().mfx_host_resample_tile(int(in_hz), int(out_hz), int(zeros), float(rolloff), int(channels)))
    if n < 0:
        raise MfxError(n, "mfx_host_resample_tile failed")
    return n


def periodic_hann(n):
    """The periodic Hann window of n taps, float32: 0.5 - 0.5 cos(2 pi j / n) (torch.hann_window(n), Whisper's at n = 400)."""
    j = np.arange(int(n), dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * j / int(n))).astype(np.float32)


def host_slaney_mel_table(num_banks, dft_size, sample_rate, low_freq, high_freq):
    """Slaney mel table of the STFT log-mel front end exactly as uploaded (host code, no GPU needed): (weights
    [num_banks][dft_size / 2 + 1], beg [num_banks], len [num_banks]) -- beg / len the non-zero span of every row."""
    L = load_library()
    w = np.zeros((int(num_banks), int(dft_size) // 2 + 1), np.float32)
    beg, ln = np.zeros(int(num_banks), np.int32), np.zeros(int(num_banks), np.int32)
    p32 = C.POINTER(C.c_int32)
    rc = L.mfx_host_slaney_mel_table(int(num_banks), int(dft_size), float(sample_rate), float(low_freq), float(high_freq),
                                     w.ctypes.data_as(C.POINTER(C.c_float)), beg.ctypes.data_as(p32), ln.ctypes.data_as(p32))
    if rc != 0:
        raise MfxError(rc, "mfx_host_slaney_mel_table failed")
    return w, beg, ln


def host_stft_basis(window):
    """Windowed DFT basis of the STFT log-mel front end exactly as uploaded (host code, no GPU needed): [2][N / 2 + 1][N] for a
    window of N taps -- the cosine rows, then the negated sine rows."""
    L = load_library()
    w = np.ascontiguousarray(window, dtype=np.float32)
    n = int(w.size)
    out = np.zeros((2, n // 2 + 1, n), np.float32)
    fpt = C.POINTER(C.c_float)
    rc = L.mfx_host_stft_basis(n, w.ctypes.data_as(fpt), out.ctypes.data_as(fpt))
    if rc != 0:
        raise MfxError(rc, "mfx_host_stft_basis failed")
    return out


def host_stft_fft_tables(dft_size):
    """Tables of the FFT form of the STFT log-mel front end (dft_size 1024 or 2048) exactly as uploaded (host code, no GPU
    needed): (twid [dft_size / 2] complex64, W_M^k of the half-length FFT; split [dft_size / 2 + 1] complex64, -i W_N^k of the
    real split)."""
    L = load_library()
    n = int(dft_size)
    twid, split = np.zeros(max(n, 0), np.float32), np.zeros(max(n, 0) + 2, np.float32)
    fpt = C.POINTER(C.c_float)
    rc = L.mfx_host_stft_fft_tables(n, twid.ctypes.data_as(fpt), split.ctypes.data_as(fpt))
    if rc != 0:
        raise MfxError(rc, "mfx_host_stft_fft_tables failed")
    return twid.view(np.complex64), split.view(np.complex64)


def host_stft_fft_lds_bytes(dft_size, shift, num_banks):
    """(LDS bytes of a block of k_stft_fft_mel, frames per block) at the tile mfx_create takes for the shape.  An inspection
    aid: the tiling is the kernel's private matter."""
    r = C.c_int32(0)
    n = int(load_library().mfx_host_stft_fft_lds_bytes(int(dft_size), int(shift), int(num_banks), C.byref(r)))
    if n < 0:
        raise MfxError(n, "mfx_host_stft_fft_lds_bytes failed")
    return n, int(r.value)


def stft_frame_count(samples, dft_size, shift):
    """Frames of an utterance of `samples` samples on an STFT log-mel handle: 0 up to dft_size / 2, else samples // shift."""
    n = int(load_library().mfx_host_stft_frame_count(int(samples), int(dft_size), int(shift)))
    if n < 0:
        raise MfxError(n, "mfx_host_stft_frame_count failed")
    return n


def povey_window(n):
    """Kaldi's default ("povey") window of n taps, float32: pow(0.5 - 0.5 cos(2 pi i / (n - 1)), 0.85), in double, rounded
    once."""
    i = np.arange(int(n), dtype=np.float64)
    return np.power(0.5 - 0.5 * np.cos(2.0 * np.pi * i / (int(n) - 1)), 0.85).astype(np.float32)


def kaldi_fft_size(window_size):
    """DFT length of a Kaldi handle: the next power of two >= window_size (128 at least)."""
    return 128 if window_size <= 128 else 256 if window_size <= 256 else 512


def host_kaldi_mel_table(num_banks, fft_size, sample_rate, low_freq, high_freq):
    """Kaldi's mel table exactly as uploaded (host code, no GPU needed): (weights [num_banks][fft_size / 2], beg [num_banks],
    len [num_banks]) -- beg / len the non-zero span of every band.  high_freq <= 0 is the offset from Nyquist."""
    L = load_library()
    w = np.zeros((max(int(num_banks), 0), max(int(fft_size), 0) // 2), np.float32)
    beg, ln = np.zeros(max(int(num_banks), 0), np.int32), np.zeros(max(int(num_banks), 0), np.int32)
    p32 = C.POINTER(C.c_int32)
    rc = L.mfx_host_kaldi_mel_table(int(num_banks), int(fft_size), float(sample_rate), float(low_freq), float(high_freq),
                                    w.ctypes.data_as(C.POINTER(C.c_float)), beg.ctypes.data_as(p32), ln.ctypes.data_as(p32))
    if rc != 0:
        raise MfxError(rc, "mfx_host_kaldi_mel_table failed")
    return w, beg, ln


def host_kaldi_dct(num_banks, ceps_len, lifter):
    """Kaldi's DCT times its lifter exactly as uploaded (host code, no GPU needed): G [ceps_len][num_banks], row 0 is c0's."""
    L = load_library()
    g = np.zeros((max(int(ceps_len), 0), max(int(num_banks), 0)), np.float32)
    rc = L.mfx_host_kaldi_dct(int(num_banks), int(ceps_len), float(lifter), g.ctypes.data_as(C.POINTER(C.c_float)))
    if rc != 0:
        raise MfxError(rc, "mfx_host_kaldi_dct failed")
    return g


def host_kaldi_lds_bytes(window_size, shift, num_banks, ceps_len, flags=0):
    """ALL the LDS bytes a block of k_kaldi_front asks for at a shape (under ``flags``, a sum of KALDI_*).  An inspection aid."""
    L = load_library()
    if flags:
        n = int(L.mfx_host_kaldi_lds_bytes_flags(int(window_size), int(shift), int(num_banks), int(ceps_len), int(flags)))
    else:
        n = int(L.mfx_host_kaldi_lds_bytes(int(window_size), int(shift), int(num_banks), int(ceps_len)))
    if n < 0:
        raise MfxError(n, "mfx_host_kaldi_lds_bytes failed")
    return n


def kaldi_flags_supported():
    """The KALDI_* bits of ``kaldi_flags`` this library serves."""
    return int(load_library().mfx_kaldi_flags_supported())


def host_kaldi_frame_count(samples, window_size, shift, flags=0):
    """Frames of an utterance on a Kaldi handle under ``flags`` (KALDI_NO_SNIP_EDGES: (n + S // 2) // S).  No GPU needed."""
    n = int(load_library().mfx_host_kaldi_frame_count(int(samples), int(window_size), int(shift), int(flags)))
    if n < 0:
        raise MfxError(n, "mfx_host_kaldi_frame_count failed")
    return n


def host_kaldi_frame_samples(samples, window_size, shift, flags, t):
    """The utterance sample index of every tap of frame ``t`` (int64 [window_size]), by the closed form the kernel uses."""
    idx = np.zeros(max(int(window_size), 0), np.int64)
    rc = load_library().mfx_host_kaldi_frame_samples(int(samples), int(window_size), int(shift), int(flags), int(t),
                                                     idx.ctypes.data_as(C.POINTER(C.c_int64)))
    if rc != 0:
        raise MfxError(rc, "mfx_host_kaldi_frame_samples failed")
    return idx


def host_frame_count(samples, window_size, shift):
    return int(load_library().mfx_host_frame_count(int(samples), int(window_size), int(shift)))


def reference_window(window_size):
    """The window the reference's caller builds (ASR_OCL.cpp:149-151):
    ``(float)(0.56f - 0.46f*cos((2.0f*M_PI*i)/W)) / 32768.f`` -- note 0.56 and a denominator of W."""
    i = np.arange(window_size, dtype=np.float64)
    inner = np.float32(0.56) - np.float32(0.46) * np.cos((2.0 * np.pi * i) / window_size)
    return (inner.astype(np.float32) / np.float32(32768.0)).astype(np.float32)


def plan_kernel(window_size, shift, num_banks, sample_rate, ceps_len, want_c0=False, dyn=DYN_NONE, fft_size=0, channels=1,
                aligned=True, engine=0, low_freq=64.0, high_freq=None, input_buffer_size=0, method=METHOD_MFCC, lpc_order=0,
                traps_len=0, traps_dct_len=0):
    """Which front-end kernel the batch entries run for a shape -- asked of a PLANNING handle (mfx_plan_create: the
    library's own configuration checks, host-built tables and LDS sums, no device, nothing computed).  Works without a
    GPU; returns the kernel's name as rocprofv3 prints it.  Raises MfxError for a configuration mfx_create refuses."""
    L = load_library()
    cfg = MfxConfig(int(input_buffer_size or 100 * shift + window_size), int(window_size), int(shift), int(num_banks),
                    float(sample_rate), float(low_freq), float(sample_rate / 2 if high_freq is None else high_freq),
                    int(ceps_len), int(bool(want_c0)), 22.0, NORM_NONE, int(dyn), 3, 3, 1, int(fft_size), int(channels), 1, 0,
                    int(engine), 0)
    _check_method(method)
    cfg.method, cfg.lpc_order = int(method), int(lpc_order)
    cfg.traps_len, cfg.traps_dct_len = int(traps_len), int(traps_dct_len)
    h = C.c_void_p()
    rc = L.mfx_plan_create(C.byref(cfg), C.byref(h))
    if rc != 0:
        raise MfxError(rc, "mfx_plan_create: " + L.mfx_status_string(rc).decode())
    try:
        L.mfx_plan_set_aligned(h, int(bool(aligned)))
        return L.mfx_dominant_kernel_name(h).decode()
    finally:
        L.mfx_destroy(h)


# Shape -> front-end kernel of the batch entries (DESIGN.md section 5 prints this table; tests/test_host.py pins it through
# plan_kernel, tests/test_parity_gpu.py checks a real handle against it).  BASELINE.json configs first, then every row of
# profiles/r03/shapes_beyond_baseline.txt and the limits of each kernel.
KERNEL_TABLE = (
    # (what, plan_kernel keyword arguments, kernel)
    ("C1  a0001.wav, 16 kHz 25/10 ms, 512 pt, 26 mel, 13 MFCC + d + dd", dict(window_size=400, shift=160, num_banks=26, sample_rate=16000.0, ceps_len=13, dyn=DYN_ACC), "k_front512"),
    ("C2 / C4  16 kHz 25/10 ms, 512 pt, 40 mel, 13 MFCC + d + dd", dict(window_size=400, shift=160, num_banks=40, sample_rate=16000.0, ceps_len=13, dyn=DYN_ACC), "k_front512"),
    ("R   reference main() defaults: 15 mel, 12 MFCC + c0, CVN", dict(window_size=400, shift=160, num_banks=15, sample_rate=16000.0, ceps_len=12, want_c0=True), "k_front512"),
    ("C3  16 kHz 25/10 ms zero padded to 1024 pt, 80 mel, 13 MFCC", dict(window_size=400, shift=160, num_banks=80, sample_rate=16000.0, ceps_len=13, fft_size=1024), "k_front1024"),
    ("C5  44.1 kHz stereo, 1102/441, 2048 pt, 128 mel, 40 MFCC + d + dd", dict(window_size=1102, shift=441, num_banks=128, sample_rate=44100.0, ceps_len=40, dyn=DYN_ACC, channels=2), "k_front2048"),
    ("C2 shape, odd shift 161 (unaligned build)", dict(window_size=400, shift=161, num_banks=40, sample_rate=16000.0, ceps_len=13, dyn=DYN_ACC, aligned=False), "k_front512"),
    ("fbank-80 at 16 kHz (80 log mel energies, no DCT), 512 pt", dict(window_size=400, shift=160, num_banks=80, sample_rate=16000.0, ceps_len=0), "k_front512"),
    ("8 kHz telephony 25/10 ms: 256 pt, zero-stuffed", dict(window_size=200, shift=80, num_banks=23, sample_rate=8000.0, ceps_len=13, dyn=DYN_ACC), "k_front512"),
    ("8 kHz stereo, 256 pt", dict(window_size=200, shift=80, num_banks=23, sample_rate=8000.0, ceps_len=13, channels=2), "k_front512"),
    ("16 kHz stereo, 512 pt", dict(window_size=400, shift=160, num_banks=40, sample_rate=16000.0, ceps_len=13, channels=2), "k_front512"),
    ("11.025 kHz 25/10 ms: 512 pt", dict(window_size=276, shift=110, num_banks=40, sample_rate=11025.0, ceps_len=13), "k_front512"),
    ("128-point transform (zero-stuffed twice over)", dict(window_size=128, shift=64, num_banks=20, sample_rate=8000.0, ceps_len=12), "k_front512"),
    ("64-point transform (zero-stuffed three times over)", dict(window_size=64, shift=32, num_banks=12, sample_rate=8000.0, ceps_len=8), "k_front512"),
    ("256 pt with the stuffed form switched off (MFX_ENGINE_NO_STUFF256)", dict(window_size=200, shift=80, num_banks=23, sample_rate=8000.0, ceps_len=13, engine=128), "k_front_wave"),
    ("512 pt, more than 128 filters", dict(window_size=400, shift=160, num_banks=160, sample_rate=16000.0, ceps_len=13), "k_front_wave"),
    ("22.05 kHz 25/10 ms: 1024 pt (552 taps, aligned frames)", dict(window_size=552, shift=220, num_banks=80, sample_rate=22050.0, ceps_len=13), "k_front1024"),
    ("22.05 kHz fbank-80 (no DCT), 1024 pt", dict(window_size=552, shift=220, num_banks=80, sample_rate=22050.0, ceps_len=0), "k_front1024"),
    ("32 kHz 25/10 ms: 1024 pt (800 taps)", dict(window_size=800, shift=320, num_banks=80, sample_rate=32000.0, ceps_len=13), "k_front1024"),
    ("C3 shape, odd shift 161 (unaligned build)", dict(window_size=400, shift=161, num_banks=80, sample_rate=16000.0, ceps_len=13, fft_size=1024, aligned=False), "k_front1024"),
    ("1024 pt, 800 taps on UNALIGNED frames", dict(window_size=800, shift=321, num_banks=80, sample_rate=32000.0, ceps_len=13, aligned=False), "k_front_reg"),
    ("1024 pt, more than 80 filters", dict(window_size=400, shift=160, num_banks=96, sample_rate=16000.0, ceps_len=13, fft_size=1024), "k_front_reg"),
    ("1024 pt, more than 16 columns with a DCT", dict(window_size=400, shift=160, num_banks=80, sample_rate=16000.0, ceps_len=20, fft_size=1024), "k_front_reg"),
    ("1024 pt stereo", dict(window_size=552, shift=220, num_banks=80, sample_rate=22050.0, ceps_len=13, channels=2), "k_front_reg"),
    ("C3 shape with k_front1024 switched off (MFX_ENGINE_NO_FRONT1024)", dict(window_size=400, shift=160, num_banks=80, sample_rate=16000.0, ceps_len=13, fft_size=1024, engine=1), "k_front_reg"),
    ("44.1 kHz mono, odd shift 441 (any-alignment build)", dict(window_size=1102, shift=441, num_banks=128, sample_rate=44100.0, ceps_len=40, dyn=DYN_ACC, aligned=False), "k_front2048"),
    ("48 kHz 25/10 ms: 2048 pt (1200 taps, 20-row build)", dict(window_size=1200, shift=480, num_banks=128, sample_rate=48000.0, ceps_len=40, dyn=DYN_ACC), "k_front2048"),
    ("n_fft = win_length = 2048, hop 512 (32-row build)", dict(window_size=2048, shift=512, num_banks=128, sample_rate=44100.0, ceps_len=40), "k_front2048"),
    ("C5 shape with k_front2048 switched off (MFX_ENGINE_NO_FRONT2048)", dict(window_size=1102, shift=441, num_banks=128, sample_rate=44100.0, ceps_len=40, dyn=DYN_ACC, channels=2, engine=4), "k_front_reg"),
    ("4096 pt (50 ms at 48 kHz): spectrum + k_melcep", dict(window_size=2400, shift=480, num_banks=64, sample_rate=48000.0, ceps_len=13), "k_front_reg"),
    ("4096 pt, 20 wide filters (ADVICE r3)", dict(window_size=2400, shift=480, num_banks=20, sample_rate=48000.0, ceps_len=12), "k_front_reg"),
    ("any shape on the streaming interface's kernels (MFX_ENGINE_STREAM_KERNELS)", dict(window_size=400, shift=160, num_banks=40, sample_rate=16000.0, ceps_len=13, dyn=DYN_ACC, engine=8), "k_front512"),
)


VAD_FLAGS, VAD_SELECT, VAD_PACK = 0, 1, 2                  # mfx_batch_set_vad modes (include/mfx.h)
PF_POV, PF_NORM_LOG_PITCH, PF_DELTA, PF_RAW_LOG_PITCH = 1, 2, 4, 8   # MFX_PF_*: columns of mfx_batch_set_pitch_feats
SPK_POOL, SPK_PRIOR_ONLY = 0, 1                            # mfx_batch_set_speakers modes (include/mfx.h)
ENGINE_NO_FRONT1024, ENGINE_FUSE_DELTA, ENGINE_NO_FRONT2048, ENGINE_STREAM_KERNELS, ENGINE_NORM_TWO_KERNELS = 1, 2, 4, 8, 16
ENGINE_DMA_SMALL_BLOCKS, ENGINE_NO_DCT_SPLIT, ENGINE_NO_STUFF256, ENGINE_FRONT1024_12_WAVES = 32, 64, 128, 256     # mfx_config.engine bits (include/mfx.h)
ENGINE_TRAPS_VALU, ENGINE_XFORM_VALU, ENGINE_SESS_NARROW_LOADS = 512, 1024, 2048
ENGINE_SESS_XFORM_PLAIN, ENGINE_SESS_STFT_PLAIN = 4096, 8192
ENGINE_FUSE_NO_SHARE, ENGINE_FUSE_SHARE_ALL, ENGINE_NO_FUSE_DELTA = 16384, 32768, 65536


class MfccHip:
    """Python mirror of ``class MfccHip : public MfccBase`` (host/afet_param.h).

    Constructor arguments are those of MfccBase (mfccbase.h:21-35) in the same order; ``device``
    replaces MfccOpenCL's trailing ``cl_device_id`` (mfccopencl.h:60).  ``method=METHOD_PLP`` computes PLP cepstra
    of model order ``lpc_order`` (0 = 8) instead of MFCC, with the same interface and output layout.
    ``method=METHOD_TRAPS`` (``ceps_len=0``, ``want_c0=False``) computes TRAPS temporal patterns: ``traps_dct_len`` (0 = 10)
    DCT coefficients of the ``traps_len`` (0 = 31) frames around each frame, per mel band -- through the batch entries
    only; the streaming methods raise ``MfxError`` (-8).
    ``method=METHOD_STFT_LOGMEL`` computes the log-mel spectrogram of the Whisper family (include/mfx.h): ``window_size`` is
    the DFT length, ``num_banks`` the output width, ``logmel_post`` one of ``LOGMEL_*``; set ``periodic_hann(window_size)``
    as the window.  Batch entries, and for ``LOGMEL_LOG10`` / ``LOGMEL_LN`` the session entries; no streaming methods.
    DFT lengths: even, 32 .. 512 (an exact matrix DFT), and 1024 / 2048 (a float32 FFT; batch entries only, the session
    entries raise ``MfxError`` (-8)).  A window shorter than the DFT (``win_length < n_fft``) is passed centred in
    ``window_size`` taps with zeros around it, left pad ``(n_fft - win_length) // 2``, as ``torch.stft`` places it.
    ``method=METHOD_KALDI`` computes Kaldi-compatible fbank (``ceps_len=0``) or MFCC (``ceps_len`` = num_ceps, c0 in column
    0; ``want_c0=False``; ``lift_coef`` = cepstral_lifter, 0 = none) features (include/mfx.h): ``window_size`` 65 .. 512,
    ``high_freq <= 0`` is Kaldi's offset from Nyquist; set ``povey_window(window_size)`` as the window and the three frame
    options with ``kaldi_set_options``.  Batch and session entries; no streaming methods, no warp factors.
    ``kaldi_flags`` (a sum of ``KALDI_NO_SNIP_EDGES``, ``KALDI_USE_ENERGY``, ``KALDI_ENERGY_WINDOWED``, ``KALDI_HTK_COMPAT``) and
    ``kaldi_energy_floor`` are Kaldi's snip_edges = false, use_energy, raw_energy = false, htk_compat and energy_floor; fbank
    with the energy column is ``num_banks + 1`` wide.  ``KALDI_NO_SNIP_EDGES``: batch entries only, no pitch track.
    """

    def __init__(self, input_buffer_size, window_size, shift, num_banks, sample_rate, low_freq, high_freq,
                 ceps_len, want_c0, lift_coef, norm=NORM_NONE, dyn=DYN_NONE, delta_l1=1, delta_l2=1,
                 norm_after_dyn=True, device=0, fft_size=0, channels=1, bug_compat=True, batch_norm_stats=0, engine=0,
                 tail_split=0, method=METHOD_MFCC, lpc_order=0, traps_len=0, traps_dct_len=0,
                 logmel_post=LOGMEL_WHISPER, kaldi_flags=0, kaldi_energy_floor=0.0):
        self._L = load_library()
        _check_method(method)
        self.cfg = MfxConfig(int(input_buffer_size), int(window_size), int(shift), int(num_banks),
                             float(sample_rate), float(low_freq), float(high_freq), int(ceps_len),
                             int(bool(want_c0)), float(lift_coef), int(norm), int(dyn), int(delta_l1),
                             int(delta_l2), int(bool(norm_after_dyn)), int(fft_size), int(channels),
                             int(bool(bug_compat)), int(batch_norm_stats), int(engine), int(tail_split),
                             int(method), int(lpc_order), int(traps_len), int(traps_dct_len), int(logmel_post))
        self.kaldi_flags, self.kaldi_energy_floor = int(kaldi_flags), float(kaldi_energy_floor)
        h = C.c_void_p()
        if int(method) == METHOD_KALDI:   # (the creation entry that carries the two options; both zero: mfx_create itself)
            rc = self._L.mfx_create_kaldi(C.byref(self.cfg), self.kaldi_flags, self.kaldi_energy_floor, int(device), C.byref(h))
        else:
            rc = self._L.mfx_create(C.byref(self.cfg), int(device), C.byref(h))
        if rc != 0:
            raise MfxError(rc, "mfx_create: " + self._L.mfx_status_string(rc).decode())
        self._h = h
        self._plan_rows = None
        self._plan_total = 0

    # -- lifetime ---------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._L.mfx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise MfxError(rc, self._L.mfx_last_error(self._h).decode() or self._L.mfx_status_string(rc).decode())

    # -- ParamBase interface (parambase.h:23-32) ----------------------------------------------------
    def get_input_buffer_size(self):
        return self._L.mfx_get_input_buffer_size(self._h)

    def estimated_window_count(self, samples):
        return self._L.mfx_estimated_window_count(self._h, int(samples))

    def set_alpha(self, alpha):
        self._chk(self._L.mfx_set_alpha(self._h, float(alpha)))

    def kaldi_set_options(self, preemph_coeff=0.97, remove_dc_offset=True, use_power=True):
        """The three frame options of a METHOD_KALDI handle (Kaldi's defaults).  Flags may be given as 0 / 1; any other
        integer is refused by the library."""
        self._chk(self._L.mfx_kaldi_set_options(self._h, float(preemph_coeff), int(remove_dc_offset), int(use_power)))

    def set_window(self, window):
        w = np.ascontiguousarray(window, dtype=np.float32)
        if w.size != self.cfg.window_size:
            raise ValueError("window must have window_size taps")
        self._chk(self._L.mfx_set_window(self._h, w.ctypes.data_as(C.POINTER(C.c_float))))

    def set_input(self, data):
        pcm = np.ascontiguousarray(data, dtype=np.int16)
        n = C.c_int32(0)
        self._chk(self._L.mfx_set_input(self._h, pcm.ctypes.data_as(C.POINTER(C.c_int16)), pcm.size, C.byref(n)))
        return n.value

    def flush(self):
        n = C.c_int32(0)
        self._chk(self._L.mfx_flush(self._h, C.byref(n)))
        return n.value

    def apply(self):
        self._chk(self._L.mfx_apply(self._h))

    def get_output_data_width(self):
        return self._L.mfx_get_output_data_width(self._h)

    def get_output_data(self, window_count):
        out = np.empty((max(int(window_count), 0), self.get_output_data_width()), dtype=np.float32)
        self._chk(self._L.mfx_get_output_data(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), int(window_count)))
        return out

    def apply_alphas(self, alphas):
        """VTLN sweep: every warp factor of `alphas` over the stored spectrum of the current block in
        one call (the reference's alpha loop, ASR_OCL.cpp:236-243)."""
        a = np.ascontiguousarray(alphas, dtype=np.float32)
        self._chk(self._L.mfx_apply_alphas(self._h, a.ctypes.data_as(C.POINTER(C.c_float)), int(a.size)))

    def get_output_data_alpha(self, alpha_index, window_count):
        out = np.empty((max(int(window_count), 0), self.get_output_data_width()), dtype=np.float32)
        self._chk(self._L.mfx_get_output_data_alpha(self._h, int(alpha_index), out.ctypes.data_as(C.POINTER(C.c_float)),
                                                    int(window_count)))
        return out

    # -- extensions ---------------------------------------------------------------------------------
    def max_frames_out(self):
        return self._L.mfx_max_frames_out(self._h)

    def fft_size(self):
        return self._L.mfx_fft_size(self._h)

    def process_stream(self, pcm, block_samples=0, alpha=1.0):
        """The per-file loop of the reference driver (ASR_OCL.cpp:227-301): blocks of at most
        get_input_buffer_size() samples through set_input/apply/get_output_data, then flush."""
        pcm = np.ascontiguousarray(pcm, dtype=np.int16)
        limit = self.get_input_buffer_size()
        if block_samples and block_samples < limit:
            limit = int(block_samples)
        rows, pos = [], 0
        while pos < pcm.size:
            n = self.set_input(pcm[pos:pos + limit])
            self.set_alpha(alpha)
            self.apply()
            rows.append(self.get_output_data(n))
            pos += limit
        n = self.flush()
        if n > 0:
            self.set_alpha(alpha)
            self.apply()
            rows.append(self.get_output_data(n))
        return np.concatenate(rows, 0) if rows else np.zeros((0, self.get_output_data_width()), np.float32)

    # -- batch interface ----------------------------------------------------------------------------
    def batch_frames(self, samples):
        return int(self._L.mfx_batch_frames(self._h, int(samples)))

    def batch_plan(self, offsets, lengths):
        off = np.ascontiguousarray(offsets, dtype=np.int64)
        ln = np.ascontiguousarray(lengths, dtype=np.int64)
        assert off.size == ln.size
        rows = np.zeros(off.size, dtype=np.int64)
        total = C.c_int64(0)
        p64 = C.POINTER(C.c_int64)
        self._chk(self._L.mfx_batch_plan(self._h, off.size, off.ctypes.data_as(p64), ln.ctypes.data_as(p64),
                                         rows.ctypes.data_as(p64), C.byref(total)))
        self._plan_rows, self._plan_total = rows, total.value
        self._pf_F = self._paste_F = 0                               # (a plan drops the attachments)
        return rows, total.value

    def batch_plan_rates(self, offsets, lengths, rates, zeros=0, rolloff=0.0):
        """batch_plan for utterances at their own sample rates (mfx_batch_plan_rates): offsets / lengths in input-rate
        samples per channel, rates in Hz; the run converts every utterance to cfg.sample_rate on the device first.
        Returns (out_rows, total_rows) of the converted lengths."""
        off = np.ascontiguousarray(offsets, dtype=np.int64)
        ln = np.ascontiguousarray(lengths, dtype=np.int64)
        rt = np.ascontiguousarray(rates, dtype=np.int32)
        assert off.size == ln.size == rt.size
        rows = np.zeros(off.size, dtype=np.int64)
        total = C.c_int64(0)
        p64 = C.POINTER(C.c_int64)
        self._chk(self._L.mfx_batch_plan_rates(self._h, off.size, off.ctypes.data_as(p64), ln.ctypes.data_as(p64),
                                               rt.ctypes.data_as(C.POINTER(C.c_int32)), int(zeros), float(rolloff),
                                               rows.ctypes.data_as(p64), C.byref(total)))
        self._plan_rows, self._plan_total = rows, total.value
        self._pf_F = self._paste_F = 0                               # (a plan drops the attachments)
        return rows, total.value

    def batch_resample_layout(self):
        """(offsets, lengths, total) of the converted PCM in output-rate samples per channel, while a rates plan is in
        force (MfxError with status -8 otherwise)."""
        n = 0 if self._plan_rows is None else self._plan_rows.size
        off, ln = np.zeros(n, np.int64), np.zeros(n, np.int64)
        total = C.c_int64(0)
        p64 = C.POINTER(C.c_int64)
        self._chk(self._L.mfx_batch_resample_layout(self._h, off.ctypes.data_as(p64), ln.ctypes.data_as(p64), C.byref(total)))
        return off, ln, total.value

    host_resample_taps = staticmethod(host_resample_taps)
    host_resampled_length = staticmethod(host_resampled_length)
    host_resample_layout = staticmethod(host_resample_layout)

    def batch_run_device(self, d_pcm_ptr, pcm_samples_total, d_out_ptr):
        """Device pointers in, device pointer out; asynchronous on the handle's stream."""
        self._chk(self._L.mfx_batch_run_device(self._h, C.c_void_p(int(d_pcm_ptr)), int(pcm_samples_total),
                                               C.c_void_p(int(d_out_ptr))))

    def batch_run_host(self, pcm):
        """The planned batch from host PCM: the ragged rows [total_rows][batch_output_width()] float32, or, while a tensor
        output is in force (batch_set_tensor), an array of the tensor's shape and type (bfloat16 as uint16 bits)."""
        pcm = np.ascontiguousarray(pcm, dtype=np.int16)
        total = pcm.size // max(self.cfg.channels, 1)
        shape = self.batch_tensor_shape()
        if shape is None:
            out = np.zeros((self._plan_total, self.batch_output_width()), dtype=np.float32)
        else:
            out = np.zeros(shape[0], dtype=shape[1])
        self._chk(self._L.mfx_batch_run_host(self._h, pcm.ctypes.data_as(C.POINTER(C.c_int16)), total,
                                             C.cast(C.c_void_p(out.ctypes.data), C.POINTER(C.c_float))))
        return out

    host_tensor_pack = staticmethod(host_tensor_pack)
    host_tensor_bytes = staticmethod(host_tensor_bytes)

    def batch_set_tensor(self, layout=TENSOR_TIME_MAJOR, dtype=DTYPE_F32, t_pad=0, pad_value=0.0):
        """Dense padded tensor output of a batch run (mfx_batch_set_tensor; set it LAST, behind the transform, the pitch
        features and the VAD): d_out becomes [B][Tp][Wo] (TENSOR_TIME_MAJOR) or [B][Wo][Tp] (TENSOR_CHANNEL_MAJOR) of
        DTYPE_F32 / DTYPE_F16 / DTYPE_BF16, Tp = t_pad or the plan's longest utterance, longer utterances cut, shorter ones
        padded with pad_value; every element is written on every run.  A later batch_plan clears it."""
        self._chk(self._L.mfx_batch_set_tensor(self._h, int(layout), int(dtype), int(t_pad), float(pad_value)))
        self._tensor_dtype = int(dtype)

    def batch_clear_tensor(self):
        self._chk(self._L.mfx_batch_clear_tensor(self._h))

    def batch_output_bytes(self):
        """Bytes a batch run writes at d_out: the tensor's while one is in force, else total_rows * batch_output_width() * 4."""
        n = int(self._L.mfx_batch_output_bytes(self._h))
        if n < 0:
            self._chk(n)
        return n

    def batch_tensor_shape(self):
        """((B, Tp, Wo) or (B, Wo, Tp), numpy dtype) of the tensor output in force (bfloat16: uint16), else None."""
        dims, eb = (C.c_int64 * 3)(), C.c_int32(0)
        rc = self._L.mfx_batch_tensor_shape(self._h, dims, C.byref(eb))
        if rc == -8:
            return None
        self._chk(rc)
        dt = np.float32 if eb.value == 4 else _TENSOR_NP[getattr(self, "_tensor_dtype", DTYPE_F16)]
        return (int(dims[0]), int(dims[1]), int(dims[2])), dt

    def batch_tensor_lengths(self):
        """len [B] int32 = min(L_u, Tp) of the tensor output in force (synchronises; MfxError with status -8 without one, or
        before a run when a selecting VAD decides the lengths)."""
        n = 0 if self._plan_rows is None else self._plan_rows.size
        ln = np.zeros(n, np.int32)
        self._chk(self._L.mfx_batch_tensor_lengths(self._h, ln.ctypes.data_as(C.POINTER(C.c_int32)), None))
        return ln

    def batch_tensor_lengths_device(self):
        """Device address of the handle-owned len [B] int32 (synchronises, as batch_tensor_lengths)."""
        a = C.c_void_p()
        self._chk(self._L.mfx_batch_tensor_lengths(self._h, None, C.byref(a)))
        return a.value or 0

    def batch_tensor_from_rows(self, d_rows_ptr, d_out_ptr):
        """The tensor launch alone (mfx_batch_tensor_from_rows): device rows [total_rows][Wo] float32 in the plan's row order
        -> the tensor at d_out_ptr; asynchronous on the handle's stream."""
        self._chk(self._L.mfx_batch_tensor_from_rows(self._h, C.c_void_p(int(d_rows_ptr)), C.c_void_p(int(d_out_ptr))))

    def batch_set_alphas(self, alphas):
        """One VTLN warp factor per utterance of the planned batch (float32 array, plan order); None clears the list.
        A later batch_plan clears it too."""
        if alphas is None:
            self._chk(self._L.mfx_batch_set_alphas(self._h, None, 0))
            return
        a = np.ascontiguousarray(alphas, dtype=np.float32)
        self._chk(self._L.mfx_batch_set_alphas(self._h, a.ctypes.data_as(C.POINTER(C.c_float)), int(a.size)))

    def batch_set_transform(self, A, b=None, left=0, right=0, utt_xf=None):
        """Splice + affine transform as the last stage of a batch run (mfx_batch_set_transform): every output row becomes
        b + A . [rows t - left .. t + right of the utterance, edges replicated].  A is [out_dim][in_dim] or
        [n_xf][out_dim][in_dim] with in_dim = (left + right + 1) * get_output_data_width(); b [out_dim] / [n_xf][out_dim] or
        None (zeros); utt_xf one transform index per planned utterance or None (all 0).  A = None clears the transform; a
        later batch_plan clears it too."""
        if A is None:
            self._chk(self._L.mfx_batch_set_transform(self._h, 0, 0, 0, 0, None, None, None, 0))
            return
        a = np.ascontiguousarray(A, dtype=np.float32)
        if a.ndim == 2:
            a = a[None]
        if a.ndim != 3:
            raise ValueError("A must be [out_dim][in_dim] or [n_xf][out_dim][in_dim]")
        n_xf, out_dim, in_dim = a.shape
        if in_dim != (int(left) + int(right) + 1) * (self.get_output_data_width() + int(getattr(self, "_paste_F", 0))):
            raise ValueError("A must have (left + right + 1) * get_output_data_width() columns (and the pasted pitch features')")
        fpt, ipt = C.POINTER(C.c_float), C.POINTER(C.c_int32)
        bb = None
        if b is not None:
            bb = np.ascontiguousarray(b, dtype=np.float32).reshape(-1)
            if bb.size != n_xf * out_dim:
                raise ValueError("b must have out_dim entries per transform")
        idx = None if utt_xf is None else np.ascontiguousarray(utt_xf, dtype=np.int32)
        self._chk(self._L.mfx_batch_set_transform(
            self._h, int(left), int(right), out_dim, n_xf, a.ctypes.data_as(fpt), None if bb is None else bb.ctypes.data_as(fpt),
            None if idx is None else idx.ctypes.data_as(ipt), 0 if idx is None else int(idx.size)))

    def norm_width(self):
        """Wn of the speaker entries: the normalised columns of a row (all of them after the deltas, else the statics)."""
        w = self.get_output_data_width()
        return w if self.cfg.norm_after_dyn else w // (1 + self.cfg.dyn)

    def batch_set_speakers(self, utt_spk, n_spk=None, prior=None, mode=SPK_POOL):
        """Per-speaker CMN / CVN / MINMAX (mfx_batch_set_speakers): utt_spk is one speaker id per planned utterance; the
        normaliser's statistics are pooled over each speaker's utterances.  n_spk: number of speakers (None: largest id +
        1); prior: (count [n_spk], acc [n_spk][4][Wn]) of an earlier batch_speaker_stats or sharding.merge_speaker_acc;
        mode SPK_PRIOR_ONLY takes the statistics from the prior alone.  utt_spk = None clears the list; a later batch_plan
        clears it too."""
        if utt_spk is None:
            self._chk(self._L.mfx_batch_set_speakers(self._h, None, 0, 0, None, None, 0))
            self._n_spk = 0
            return
        ids = np.ascontiguousarray(utt_spk, dtype=np.int32)
        if n_spk is None:
            n_spk = int(ids.max()) + 1 if ids.size else 1
        n_spk = int(n_spk)
        pc = pa = None
        if prior is not None:
            pc = np.ascontiguousarray(prior[0], dtype=np.int64)
            pa = np.ascontiguousarray(prior[1], dtype=np.float64)
            if pc.size != n_spk or pa.size != n_spk * 4 * self.norm_width():
                raise ValueError("prior must be (count [n_spk], acc [n_spk][4][Wn])")
        self._chk(self._L.mfx_batch_set_speakers(
            self._h, ids.ctypes.data_as(C.POINTER(C.c_int32)), int(ids.size), n_spk,
            None if pc is None else pc.ctypes.data_as(C.POINTER(C.c_int64)),
            None if pa is None else pa.ctypes.data_as(C.POINTER(C.c_double)), int(mode)))
        self._n_spk = n_spk

    def batch_speaker_stats(self):
        """(count [n_spk] int64, acc [n_spk][4][Wn] float64 = S, S2, min, max, stats [n_spk][2][Wn] float32 = mean,
        multiplier) the last batch run used, while a speaker list is in force (MfxError with status -8 otherwise)."""
        n, wn = int(getattr(self, "_n_spk", 0)), self.norm_width()
        count = np.zeros(n, np.int64)
        acc = np.zeros((n, 4, wn), np.float64)
        stats = np.zeros((n, 2, wn), np.float32)
        self._chk(self._L.mfx_batch_speaker_stats(self._h, count.ctypes.data_as(C.POINTER(C.c_int64)),
                                                  acc.ctypes.data_as(C.POINTER(C.c_double)),
                                                  stats.ctypes.data_as(C.POINTER(C.c_float))))
        return count, acc, stats

    host_speaker_lists = staticmethod(host_speaker_lists)

    def _online_args(self, window, prior_frames, prior):
        pc, pa = 0, None
        if prior is not None:
            pc = int(prior[0])
            pa = np.ascontiguousarray(prior[1], dtype=np.float64)
            if pa.size != 2 * self.norm_width():
                raise ValueError("prior must be (count, acc [2][Wn])")
        return (int(window), int(prior_frames), pc, None if pa is None else pa.ctypes.data_as(C.POINTER(C.c_double))), pa

    def batch_set_online_norm(self, window=0, prior_frames=0, prior=None):
        """Online (causal) CMN / CVN of the planned batch (mfx_batch_set_online_norm): every row is normalised with the
        statistics of the last `window` rows of its utterance, itself included (0: of all rows so far; else a multiple of 32
        up to 4096), smoothed with up to prior_frames frames of prior = (count, acc [2][Wn] = sum, sum of squares).  A later
        batch_plan clears it."""
        args, keep = self._online_args(window, prior_frames, prior)
        self._chk(self._L.mfx_batch_set_online_norm(self._h, *args))

    def batch_clear_online_norm(self):
        self._chk(self._L.mfx_batch_clear_online_norm(self._h))

    def sessions_set_online_norm(self, window=0, prior_frames=0, prior=None):
        """The same normaliser on the session entries (mfx_sessions_set_online_norm): call it before sessions_create; every
        push then delivers the bits a batch run with batch_set_online_norm of the same parameters gives the whole stream."""
        args, keep = self._online_args(window, prior_frames, prior)
        self._chk(self._L.mfx_sessions_set_online_norm(self._h, *args))

    def sessions_clear_online_norm(self):
        self._chk(self._L.mfx_sessions_clear_online_norm(self._h))

    host_online_norm = staticmethod(host_online_norm)

    def batch_set_sliding_norm(self, window=600, min_window=100, center=False, norm_vars=False):
        """Sliding-window CMN / CVN of the planned batch (mfx_batch_set_sliding_norm; the defaults are apply-cmvn-sliding's):
        every row of a norm = NONE handle is normalised with the statistics of `window` rows of its utterance around it
        (center) or behind it, between the rows y and the transform; the VAD keeps deciding on the raw rows.  A later
        batch_plan clears it."""
        self._chk(self._L.mfx_batch_set_sliding_norm(self._h, int(window), int(min_window), int(bool(center)), int(bool(norm_vars))))

    def batch_clear_sliding_norm(self):
        self._chk(self._L.mfx_batch_clear_sliding_norm(self._h))

    host_sliding_window = staticmethod(host_sliding_window)
    host_sliding_norm = staticmethod(host_sliding_norm)

    def batch_set_vad(self, column=-1, energy_threshold=5.0, energy_mean_scale=0.5, frames_context=0,
                      proportion_threshold=0.6, mode=VAD_FLAGS):
        """Energy VAD as the last stage of a batch run (mfx_batch_set_vad; the defaults are compute-vad-energy's): frame t
        is voiced when at least proportion_threshold of the frames within frames_context of it (inside the utterance) have
        column `column` (-1: the last static column) above energy_threshold + energy_mean_scale * the utterance's mean.
        VAD_FLAGS leaves the rows alone; VAD_SELECT moves every utterance's voiced rows to the front of its row range;
        VAD_PACK packs the whole batch's voiced rows; what is left over is zero.  A later batch_plan clears it."""
        self._chk(self._L.mfx_batch_set_vad(self._h, int(column), float(energy_threshold), float(energy_mean_scale),
                                            int(frames_context), float(proportion_threshold), int(mode)))

    def batch_clear_vad(self):
        self._chk(self._L.mfx_batch_clear_vad(self._h))

    def batch_vad_read(self):
        """(flags [total_rows] uint8, voiced [n_utt] int32, threshold [n_utt] float32, total_voiced) of the last batch run,
        while a VAD is in force (MfxError with status -8 otherwise)."""
        n = 0 if self._plan_rows is None else self._plan_rows.size
        flags = np.zeros(int(self._plan_total or 0), np.uint8)
        voiced, thr = np.zeros(n, np.int32), np.zeros(n, np.float32)
        total = C.c_int64(0)
        self._chk(self._L.mfx_batch_vad_read(self._h, flags.ctypes.data_as(C.POINTER(C.c_uint8)),
                                             voiced.ctypes.data_as(C.POINTER(C.c_int32)),
                                             thr.ctypes.data_as(C.POINTER(C.c_float)), C.byref(total)))
        return flags, voiced, thr, total.value

    def batch_vad_device(self):
        """Device addresses (d_flags, d_voiced, d_packed_row0) of the handle-owned arrays of the VAD in force."""
        a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._chk(self._L.mfx_batch_vad_device(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value or 0, b.value or 0, c.value or 0

    host_pitch = staticmethod(host_pitch)

    def batch_set_pitch(self, lag_min, lag_max, window=0, ballast=0.0, lag_cost=0.0, penalty=0.0, max_jump=0):
        """Pitch track beside the rows of a batch run (mfx_batch_set_pitch): per frame the normalised cross-correlation of
        `window` samples (0: the handle's window_size) at lags lag_min .. lag_max samples, and a Viterbi path through it
        (local cost 1 - rho (1 - lag_cost lag / lag_max), transition cost penalty (ln lag - ln lag')^2 over at most max_jump
        lags, 0: any).  The rows of the run are unchanged; batch_pitch_read returns the track.  A later batch_plan clears it."""
        self._chk(self._L.mfx_batch_set_pitch(self._h, int(window), int(lag_min), int(lag_max), float(ballast), float(lag_cost),
                                              float(penalty), int(max_jump)))
        self._pitch_K = int(lag_max) - int(lag_min) + 1

    def batch_clear_pitch(self):
        self._chk(self._L.mfx_batch_clear_pitch(self._h))
        self._pitch_K = 0
        self._pf_F = self._paste_F = 0                               # (the pitch features go with the track)

    host_pitch_feats = staticmethod(host_pitch_feats)

    def batch_set_pitch_feats(self, columns=0, left=75, right=75, delta_window=2, pov_scale=2.0, pov_offset=0.0, pitch_scale=2.0,
                              delta_scale=10.0, paste=False):
        """Kaldi's pitch features from the pitch track (mfx_batch_set_pitch_feats; needs batch_set_pitch): columns is a sum of
        PF_POV, PF_NORM_LOG_PITCH, PF_DELTA, PF_RAW_LOG_PITCH (0: the first three, process-kaldi-pitch-feats' default, as
        are the other defaults).  batch_pitch_feats_read returns them; with paste they are also the last F columns of every
        row of a run, ahead of the transform and the VAD.  A later batch_plan clears it."""
        self._chk(self._L.mfx_batch_set_pitch_feats(self._h, int(columns), int(left), int(right), int(delta_window), float(pov_scale),
                                                    float(pov_offset), float(pitch_scale), float(delta_scale), 1 if paste else 0))
        self._pf_F = _pf_count(columns)
        self._paste_F = self._pf_F if paste else 0

    def batch_clear_pitch_feats(self):
        self._chk(self._L.mfx_batch_clear_pitch_feats(self._h))
        self._pf_F = self._paste_F = 0

    def batch_pitch_feats_read(self):
        """feats [total_rows][F] float32 of the last batch run while pitch features are in force (MfxError with status -8
        otherwise), indexed by the plan's rows."""
        d, F = self.batch_pitch_feats_device()
        out = np.zeros((int(self._plan_total or 0), F), np.float32)
        self._chk(self._L.mfx_batch_pitch_feats_read(self._h, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def batch_pitch_feats_device(self):
        """(device address of feats [total_rows][F], F) of the handle-owned array of the pitch features."""
        a, F = C.c_void_p(), C.c_int32(0)
        self._chk(self._L.mfx_batch_pitch_feats_device(self._h, C.byref(a), C.byref(F)))
        return a.value or 0, int(F.value)

    def batch_pitch_read(self, nccf=False, f0=False):
        """(lag [total_rows] float32, rho [total_rows] float32, index [total_rows] int32) of the last batch run while a pitch
        track is in force (MfxError with status -8 otherwise), followed by the NCCF rows [total_rows][K] and by f0 =
        sample_rate / lag in Hz (float64) when asked for."""
        rows = int(self._plan_total or 0)
        pitch, index = np.zeros((rows, 2), np.float32), np.zeros(rows, np.int32)
        K = int(getattr(self, "_pitch_K", 0))
        if nccf and K < 1:   # (the row width is this wrapper's knowledge: the track was not set through batch_set_pitch)
            raise MfxError(-8, "batch_pitch_read: no pitch track was set through batch_set_pitch")
        rho = np.zeros((rows, K), np.float32) if nccf else None
        fpt = C.POINTER(C.c_float)
        self._chk(self._L.mfx_batch_pitch_read(self._h, pitch.ctypes.data_as(fpt), index.ctypes.data_as(C.POINTER(C.c_int32)),
                                               None if rho is None else rho.ctypes.data_as(fpt)))
        out = [pitch[:, 0].copy(), pitch[:, 1].copy(), index]
        if nccf:
            out.append(rho)
        if f0:
            out.append(float(self.cfg.sample_rate) / pitch[:, 0].astype(np.float64))
        return tuple(out)

    def batch_pitch_device(self):
        """Device addresses (d_pitch [total_rows][2], d_index [total_rows]) of the handle-owned arrays of the pitch track."""
        a, b = C.c_void_p(), C.c_void_p()
        self._chk(self._L.mfx_batch_pitch_device(self._h, C.byref(a), C.byref(b)))
        return a.value or 0, b.value or 0

    def batch_output_width(self):
        """Row width of the batch entries' output: out_dim while a transform is in force, else get_output_data_width()."""
        return self._L.mfx_batch_output_width(self._h)

    # -- session entries ----------------------------------------------------------------------------
    def sessions_create(self, n_sessions, max_push_samples):
        """Size the session entries: n_sessions open streams, at most max_push_samples samples per channel per push and
        session.  Drops all session state; (0, 0) releases everything."""
        self._chk(self._L.mfx_sessions_create(self._h, int(n_sessions), int(max_push_samples)))
        self._sess_total = 0

    def sessions_reset(self, session=-1):
        """Drop the carried state of one session (-1: of all), and any pending plan."""
        self._chk(self._L.mfx_sessions_reset(self._h, int(session)))

    def sessions_plan(self, ids, offsets, lengths, final=None):
        """One push: session ids[i] receives samples [offsets[i], offsets[i] + lengths[i]) of the one PCM array of the run
        (per channel); final[i] ends its stream.  Returns (out_rows, counts, total)."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        off = np.ascontiguousarray(offsets, dtype=np.int64)
        ln = np.ascontiguousarray(lengths, dtype=np.int64)
        assert ids.size == off.size == ln.size
        fin = None if final is None else np.ascontiguousarray(final, dtype=np.int32)
        assert fin is None or fin.size == ids.size
        rows = np.zeros(ids.size, dtype=np.int64)
        counts = np.zeros(ids.size, dtype=np.int32)
        total = C.c_int64(0)
        p32, p64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
        self._chk(self._L.mfx_sessions_plan(self._h, ids.size, ids.ctypes.data_as(p32), off.ctypes.data_as(p64),
                                            ln.ctypes.data_as(p64), None if fin is None else fin.ctypes.data_as(p32),
                                            rows.ctypes.data_as(p64), counts.ctypes.data_as(p32), C.byref(total)))
        self._sess_total = total.value
        return rows, counts, total.value

    def sessions_run_device(self, d_pcm_ptr, pcm_samples_total, d_out_ptr):
        """Run the planned push on device pointers; asynchronous on the handle's stream."""
        self._chk(self._L.mfx_sessions_run_device(self._h, C.c_void_p(int(d_pcm_ptr)), int(pcm_samples_total),
                                                  C.c_void_p(int(d_out_ptr))))

    def sessions_run_host(self, pcm):
        """Run the planned push from / to host arrays; returns its rows [total][sessions_output_width()]."""
        pcm = np.ascontiguousarray(pcm, dtype=np.int16)
        total = pcm.size // max(self.cfg.channels, 1)
        out = np.zeros((getattr(self, "_sess_total", 0), self.sessions_output_width()), dtype=np.float32)
        self._chk(self._L.mfx_sessions_run_host(self._h, pcm.ctypes.data_as(C.POINTER(C.c_int16)), total,
                                                out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def sessions_delivered(self, session):
        """Rows the session has delivered since it was opened (0 for a fresh one)."""
        n = int(self._L.mfx_sessions_delivered(self._h, int(session)))
        if n < 0:
            raise MfxError(n, self._L.mfx_status_string(n).decode())
        return n

    def sessions_set_transform(self, A, b=None, left=0, right=0):
        """Splice + affine transform as the last stage of every push (mfx_sessions_set_transform): call it before
        sessions_create.  A is [out_dim][in_dim] or [n_xf][out_dim][in_dim] with in_dim = (left + right + 1) *
        get_output_data_width(); b [out_dim] / [n_xf][out_dim] or None (zeros).  A session then delivers rows [0, Ex), Ex =
        max(0, E - right) while open, and its rows are sessions_output_width() wide."""
        a = np.ascontiguousarray(A, dtype=np.float32)
        if a.ndim == 2:
            a = a[None]
        if a.ndim != 3:
            raise ValueError("A must be [out_dim][in_dim] or [n_xf][out_dim][in_dim]")
        n_xf, out_dim, in_dim = a.shape
        if in_dim != (int(left) + int(right) + 1) * self.get_output_data_width():
            raise ValueError("A must have (left + right + 1) * get_output_data_width() columns")
        fpt = C.POINTER(C.c_float)
        bb = None
        if b is not None:
            bb = np.ascontiguousarray(b, dtype=np.float32).reshape(-1)
            if bb.size != n_xf * out_dim:
                raise ValueError("b must have out_dim entries per transform")
        self._chk(self._L.mfx_sessions_set_transform(self._h, int(left), int(right), out_dim, n_xf, a.ctypes.data_as(fpt),
                                                     None if bb is None else bb.ctypes.data_as(fpt)))

    def sessions_clear_transform(self):
        self._chk(self._L.mfx_sessions_clear_transform(self._h))

    def sessions_select_transform(self, session, xf):
        """The transform of one (fresh) session; kept across final pushes and sessions_reset."""
        self._chk(self._L.mfx_sessions_select_transform(self._h, int(session), int(xf)))

    def sessions_output_width(self):
        """Row width of the session entries' output: out_dim while a session transform is set, else get_output_data_width()."""
        w = int(self._L.mfx_sessions_output_width(self._h))
        if w < 0:
            raise MfxError(w, self._L.mfx_status_string(w).decode())
        return w

    def sessions_set_rates(self, rates, zeros=0, rolloff=0.0):
        """Per-session sample-rate conversion in front of every push (mfx_sessions_set_rates): call it before
        sessions_create.  rates: up to 16 input rates in Hz (cfg.sample_rate itself is a pass-through); a session takes
        rates[0] unless sessions_select_rate says otherwise.  max_push_samples, offsets and lengths are then in input-rate
        samples per channel."""
        rt = np.ascontiguousarray(rates, dtype=np.int32).reshape(-1)
        self._chk(self._L.mfx_sessions_set_rates(self._h, rt.size, rt.ctypes.data_as(C.POINTER(C.c_int32)), int(zeros),
                                                 float(rolloff)))

    def sessions_clear_rates(self):
        self._chk(self._L.mfx_sessions_clear_rates(self._h))

    def sessions_select_rate(self, session, rate_index):
        """The rate of one (fresh) session; kept across final pushes and sessions_reset."""
        self._chk(self._L.mfx_sessions_select_rate(self._h, int(session), int(rate_index)))

    def sessions_converted_read(self, n_pieces):
        """The converted samples of the last push that ran, one int16 array [samples][channels] per piece of its plan
        (test / inspection aid; synchronises).  MfxError(ERR_STATE) when that push queued no conversion launch."""
        need = int(self._L.mfx_sessions_converted_read(self._h, None, 0, None, None))
        if need < 0:
            self._chk(need)
        ch = max(self.cfg.channels, 1)
        dst = np.zeros(max(need, 1), dtype=np.int16)
        off = np.zeros(int(n_pieces), dtype=np.int64)
        ln = np.zeros(int(n_pieces), dtype=np.int64)
        p64 = C.POINTER(C.c_int64)
        got = int(self._L.mfx_sessions_converted_read(self._h, dst.ctypes.data_as(C.POINTER(C.c_int16)), need,
                                                      off.ctypes.data_as(p64), ln.ctypes.data_as(p64)))
        if got < 0:
            self._chk(got)
        return [dst[int(o) * ch:int(o + n) * ch].reshape(-1, ch).copy() for o, n in zip(off, ln)]

    host_session_step = staticmethod(host_session_step)
    host_session_resample_step = staticmethod(host_session_resample_step)
    host_session_xform_step = staticmethod(host_session_xform_step)
    host_session_stft_step = staticmethod(host_session_stft_step)

    def batch_overlap(self, enable=True):
        """Let the delta tail of a batch overlap the next batch's front end (results complete after synchronize())."""
        self._chk(self._L.mfx_batch_overlap(self._h, int(bool(enable))))

    def set_stream(self, hip_stream_handle):
        self._chk(self._L.mfx_set_stream(self._h, C.c_void_p(int(hip_stream_handle))))

    def synchronize(self):
        self._chk(self._L.mfx_synchronize(self._h))

    def profile_enable(self, on=True):
        self._chk(self._L.mfx_profile_enable(self._h, int(bool(on))))

    def profile_read(self, reset=True):
        n, ms = C.c_int32(0), C.c_double(0)
        self._chk(self._L.mfx_profile_read(self._h, C.byref(n), C.byref(ms), int(bool(reset))))
        return n.value, ms.value

    def dominant_kernel_name(self):
        return self._L.mfx_dominant_kernel_name(self._h).decode()

    def batch_fuse_info(self):
        """(planned, share, fused launches so far, frames from / up to which a batch fuses unasked): mfx_batch_fuse_info"""
        planned, share, runs, lo, hi = C.c_int32(0), C.c_int32(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._chk(self._L.mfx_batch_fuse_info(self._h, C.byref(planned), C.byref(share), C.byref(runs), C.byref(lo), C.byref(hi)))
        return bool(planned.value), share.value, runs.value, lo.value, hi.value

    def debug_read(self, kind):
        W2, nb = self.fft_size(), self.cfg.num_banks
        dl = self.cfg.ceps_len + (1 if self.cfg.want_c0 else 0)
        if kind == 1:
            buf = np.zeros(nb + 2, dtype=np.int32)
        elif kind == 0:
            buf = np.zeros(2 * W2, dtype=np.float32)
        elif kind == 2:
            buf = np.zeros(max(nb * dl, 1), dtype=np.float32)
        elif kind == 8:   # converted PCM of the last batch run under a rates plan (int16, scratch layout)
            try:
                total = self.batch_resample_layout()[2]
            except MfxError:
                total = 0
            buf = np.zeros(max(total * max(self.cfg.channels, 1), 1), dtype=np.int16)
        else:
            buf = np.zeros(64 * 1024 * 1024 // 4, dtype=np.float32)
        n = self._L.mfx_debug_read(self._h, int(kind), buf.ctypes.data_as(C.c_void_p), buf.nbytes)
        if n < 0:
            raise MfxError(int(n), "mfx_debug_read failed")
        return buf[:n].copy()
