"""asr-featext-opencl_amd -- MI355X (gfx950) MFCC front end.

Python side of the drop-in boundary: thin ctypes bindings over ``libmfcchip.so`` (the C ABI of
``include/mfx.h``).  The compiled host mirror of the reference's ``ParamBase``/``MfccBase`` classes
lives in ``host/`` (C++); this module offers the same interface to Python callers and tests.

There is no CPU fallback here: if the shared library is missing or no HIP device is present the
constructors raise.  (The directory name is not an importable identifier; load it with
``importlib`` as ``__graft_entry__.load_package()`` does, or put the parent directory on
``sys.path`` and use ``importlib.import_module("asr-featext-opencl_amd")``.)
"""
from . import mfcc  # noqa: F401
from . import sharding  # noqa: F401
from .mfcc import (  # noqa: F401
    DYN_ACC,
    DYN_DELTA,
    DYN_NONE,
    METHOD_MFCC,
    METHOD_PLP,
    METHOD_TRAPS,
    METHOD_STFT_LOGMEL,
    LOGMEL_WHISPER,
    LOGMEL_LOG10,
    LOGMEL_LN,
    NORM_CMN,
    NORM_CVN,
    NORM_MINMAX,
    NORM_NONE,
    MfccHip,
    MfxConfig,
    MfxError,
    host_dct_matrix,
    host_dct_mfma_operands,
    host_frame_count,
    host_mel_lane_plan,
    host_mel_table,
    host_plp_tables,
    host_session_step,
    host_speaker_lists,
    host_online_norm,
    host_pitch,
    host_pitch_feats,
    PF_POV,
    PF_NORM_LOG_PITCH,
    PF_DELTA,
    PF_RAW_LOG_PITCH,
    SPK_POOL,
    SPK_PRIOR_ONLY,
    VAD_FLAGS,
    VAD_SELECT,
    VAD_PACK,
    TENSOR_TIME_MAJOR,
    TENSOR_CHANNEL_MAJOR,
    DTYPE_F32,
    DTYPE_F16,
    DTYPE_BF16,
    host_tensor_pack,
    host_tensor_bytes,
    host_tensor_tile,
    host_traps_basis,
    host_slaney_mel_table,
    host_stft_basis,
    host_stft_fft_tables,
    host_stft_fft_lds_bytes,
    stft_frame_count,
    periodic_hann,
    host_xform_operands,
    KERNEL_TABLE,
    library_path,
    load_library,
    method_supported,
    plan_kernel,
    reference_window,
)
