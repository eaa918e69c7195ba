"""ctypes binding of libneutts_hip.so (include/neutts_hip.h) + thin host-side engine wrappers.

This is the only place the product touches native code.  There is NO CPU fallback: if the
library is missing it must be built (`python neutts-air_amd/build.py`), and if no gfx950 device is
present `ntts_backbone_create` fails with NTTS_ENODEV and we raise.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import Dict, Iterable, List, Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(os.path.dirname(_HERE), "libneutts_hip.so")

NTTS_DT_F32, NTTS_DT_BF16, NTTS_DT_I32, NTTS_DT_FP8_E4M3 = 0, 1, 2, 3
NTTS_W_BF16, NTTS_W_FP8_E4M3 = 0, 1
ABI_VERSION = 11
NTTS_PAGE_TOKENS = 32            # include/neutts_hip.h
PAGE_TOKENS = 32
ERRORS = {-1: "EINVAL", -2: "ENODEV", -3: "ENOMEM", -4: "ESTATE", -5: "EHIP"}


class NeuTTSHipError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libneutts_hip: {ERRORS.get(code, code)}: {msg}")
        self.code = code


class BackboneConfigC(C.Structure):
    _fields_ = [("vocab_size", C.c_int32), ("hidden_size", C.c_int32), ("intermediate_size", C.c_int32),
                ("num_layers", C.c_int32), ("num_heads", C.c_int32), ("num_kv_heads", C.c_int32),
                ("head_dim", C.c_int32), ("rms_eps", C.c_float), ("max_context", C.c_int32),
                ("max_batch", C.c_int32), ("num_pages", C.c_int32), ("max_prefill_tokens", C.c_int32),
                ("tie_word_embeddings", C.c_int32), ("attention_bias", C.c_int32), ("qk_norm", C.c_int32),
                ("weight_dtype", C.c_int32), ("park_slots", C.c_int32)]


class CodecConfigC(C.Structure):
    _fields_ = [("hidden_size", C.c_int32), ("intermediate_size", C.c_int32), ("num_layers", C.c_int32),
                ("num_heads", C.c_int32), ("head_dim", C.c_int32), ("quantization_dim", C.c_int32),
                ("n_levels", C.c_int32), ("levels", C.c_int32 * 8), ("hop_length", C.c_int32), ("rms_eps", C.c_float),
                ("max_frames", C.c_int32), ("max_rows", C.c_int32), ("precision", C.c_int32)]


class WavFormatC(C.Structure):
    _fields_ = [("sample_rate", C.c_int32), ("encoding", C.c_int32), ("filter_width", C.c_int32)]


class WavLoudnessC(C.Structure):
    _fields_ = [("enable", C.c_int32), ("target_lufs", C.c_float), ("peak_dbfs", C.c_float), ("max_gain_db", C.c_float)]


class EncoderConfigC(C.Structure):
    _fields_ = [("sem_hidden", C.c_int32), ("sem_layers", C.c_int32), ("sem_heads", C.c_int32), ("sem_ffn", C.c_int32),
                ("sem_conv_kernel", C.c_int32), ("sem_left", C.c_int32), ("sem_right", C.c_int32), ("sem_ln_eps", C.c_float),
                ("ac_hidden", C.c_int32), ("n_ratios", C.c_int32), ("ratios", C.c_int32 * 8), ("codec_hidden", C.c_int32),
                ("n_levels", C.c_int32), ("levels", C.c_int32 * 8), ("max_samples", C.c_int32)]


class StreamParamsC(C.Structure):
    _fields_ = [("chunk", C.c_int32), ("lookforward", C.c_int32), ("lookback", C.c_int32), ("overlap", C.c_int32),
                ("hop_length", C.c_int32), ("speech_base", C.c_int32), ("n_codes", C.c_int32), ("modulo", C.c_int32)]


class SamplingC(C.Structure):
    _fields_ = [("max_length", C.c_int32), ("min_new_tokens", C.c_int32), ("eos_token_id", C.c_int32),
                ("do_sample", C.c_int32), ("top_k", C.c_int32), ("temperature", C.c_float), ("seed", C.c_uint64),
                ("top_p", C.c_float), ("min_p", C.c_float), ("repetition_penalty", C.c_float), ("prompt_ignore_length", C.c_int32)]


_LIBS: Dict[str, C.CDLL] = {}


def load_library(path: Optional[str] = None) -> C.CDLL:
    path = os.path.abspath(path or os.environ.get("NEUTTS_HIP_LIB", DEFAULT_LIB))
    if path in _LIBS:
        return _LIBS[path]
    if not os.path.exists(path):
        raise FileNotFoundError(
            f"{path} not found: build it with `python neutts-air_amd/build.py` (hipcc, gfx950). "
            "There is no CPU fallback for the NeuTTS hot path.")
    # Load order matters: PyTorch-ROCm bundles its own libamdhip64.so (SONAME libamdhip64.so.7).  If this library
    # were dlopen'ed first it would pull /opt/rocm's copy in, torch would later load its bundled one, and the process
    # would hold TWO HIP runtimes (the second one sees no devices).  Importing torch first makes both share one.
    try:
        import torch  # noqa: F401  (plumbing only)
    except ImportError:
        pass
    lib = C.CDLL(path)
    p, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    sig = {
        "ntts_abi_version": (C.c_int, []),
        "ntts_last_error": (C.c_char_p, [p]),
        "ntts_backbone_create": (C.c_int, [C.POINTER(BackboneConfigC), C.c_int, C.POINTER(p)]),
        "ntts_backbone_destroy": (None, [p]),
        "ntts_backbone_load_tensor": (C.c_int, [p, C.c_char_p, p, C.c_int, C.POINTER(i64), C.c_int, C.c_int]),
        "ntts_backbone_finalize": (C.c_int, [p]),
        "ntts_backbone_arena": (C.c_int, [p, C.POINTER(p), C.POINTER(C.c_size_t)]),
        "ntts_backbone_adopt_arena": (C.c_int, [p]),
        "ntts_backbone_arena_derived": (C.c_int, [p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
        "ntts_backbone_arena_copy": (C.c_int, [p, p, C.c_size_t, C.c_int]),
        "ntts_backbone_share_arena": (C.c_int, [p, p]),
        "ntts_backbone_set_prefill_stream": (C.c_int, [p, p]),
        "ntts_backbone_time_kernel": (C.c_int, [p, i32, i32, C.POINTER(f32), C.POINTER(C.c_double), C.POINTER(i32)]),
        "ntts_backbone_prefill": (C.c_int, [p, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(SamplingC)]),
        "ntts_backbone_prefill_shared": (C.c_int, [p, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(SamplingC),
                                                   C.POINTER(i32), C.POINTER(i32)]),
        "ntts_backbone_set_gang": (C.c_int, [p, i32]),
        "ntts_backbone_activate": (C.c_int, [p, i32, C.POINTER(i32), C.POINTER(i32)]),
        "ntts_backbone_set_logits_range": (C.c_int, [p, i32, i32, i32]),
        "ntts_backbone_calibrate": (C.c_int, [p, i32]),
        "ntts_backbone_read_amax": (C.c_int, [p, C.POINTER(f32), i32]),
        "ntts_backbone_kv_stats": (C.c_int, [p, C.POINTER(i32), C.POINTER(i32), C.POINTER(i64), C.POINTER(i64)]),
        "ntts_backbone_decode": (C.c_int, [p, i32]),
        "ntts_backbone_read": (C.c_int, [p, i32, C.POINTER(i32), i32, C.POINTER(i32), C.POINTER(i32)]),
        "ntts_backbone_read_all": (C.c_int, [p, C.POINTER(i32), i32, C.POINTER(i32), C.POINTER(i32)]),
        "ntts_backbone_poll": (C.c_int, [p, C.POINTER(i32), C.POINTER(i32)]),
        "ntts_backbone_poll_begin": (C.c_int, [p]),
        "ntts_backbone_poll_end": (C.c_int, [p, C.POINTER(i32), C.POINTER(i32)]),
        "ntts_backbone_read_finished": (C.c_int, [p, i32, C.POINTER(i32), i32, C.POINTER(i32)]),
        "ntts_backbone_release": (C.c_int, [p, i32]),
        "ntts_backbone_release_many": (C.c_int, [p, i32, C.POINTER(i32)]),
        "ntts_backbone_export_codes": (C.c_int, [p, i32, C.POINTER(i32), i32, i32, i32, p, i32, p]),
        "ntts_backbone_stream": (C.c_int, [p, C.POINTER(p)]),
        "ntts_backbone_set_stream": (C.c_int, [p, p]),
        "ntts_codec_set_stream": (C.c_int, [p, p]),
        "ntts_backbone_append_codes": (C.c_int, [p, i32, C.POINTER(i32), i32, i32, i32, p, i32, p, p, p]),
        "ntts_codec_stream": (C.c_int, [p, C.POINTER(p)]),
        "ntts_codec_set_debug": (C.c_int, [p, i32]),
        "ntts_codec_read_stage": (C.c_int, [p, i32, i32, C.POINTER(f32), i64, C.POINTER(i32), C.POINTER(i32)]),
        "ntts_codec_limits": (C.c_int, [p, C.POINTER(i32), C.POINTER(i64)]),
        "ntts_streams_last_error": (C.c_char_p, [p]),
        "ntts_streams_create": (C.c_int, [p, p, C.POINTER(StreamParamsC), i32, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), i32, C.POINTER(p)]),
        "ntts_streams_destroy": (None, [p]),
        "ntts_streams_pump_begin": (C.c_int, [p]),
        "ntts_streams_pump_wait": (C.c_int, [p, C.POINTER(i32)]),
        "ntts_streams_pump_end": (C.c_int, [p, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(C.POINTER(f32)),
                                            C.POINTER(i64), C.POINTER(i32), C.POINTER(i32)]),
        "ntts_streams_done": (C.c_int, [p, C.POINTER(i32)]),
        "ntts_codec_decode_dev": (C.c_int, [p, i32, p, i32, C.POINTER(i32), p, i64, i32, p]),
        "ntts_codec_sync": (C.c_int, [p]),
        "ntts_codec_set_cu_mask": (C.c_int, [p, C.POINTER(C.c_uint32), i32]),
        "ntts_backbone_set_prefill_cu_mask": (C.c_int, [p, C.POINTER(C.c_uint32), i32]),
        "ntts_backbone_sync": (C.c_int, [p]),
        "ntts_backbone_set_debug": (C.c_int, [p, i32]),
        "ntts_backbone_read_logits": (C.c_int, [p, i32, C.POINTER(f32), i32]),
        "ntts_backbone_read_seen": (C.c_int, [p, i32, C.POINTER(C.c_uint32), i32]),
        "ntts_backbone_set_logprobs": (C.c_int, [p, i32]),
        "ntts_backbone_read_logprobs": (C.c_int, [p, i32, C.POINTER(f32), i32, C.POINTER(i32)]),
        "ntts_backbone_read_finished_logprobs": (C.c_int, [p, i32, C.POINTER(f32), i32, C.POINTER(i32)]),
        "ntts_backbone_score": (C.c_int, [p, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), i32, C.POINTER(f32),
                                          C.POINTER(i32), C.POINTER(f32), i64, C.POINTER(i64)]),
        "ntts_backbone_read_score_logits": (C.c_int, [p, i64, C.POINTER(f32), i32]),
        "ntts_backbone_debug_force": (C.c_int, [p, i32, i32]),
        "ntts_backbone_last_timing": (C.c_int, [p, C.POINTER(f32), C.POINTER(f32)]),
        "ntts_backbone_step_bytes": (C.c_int, [p, C.POINTER(C.c_double)]),
        "ntts_backbone_attn_timeline": (C.c_int, [p, i32, C.POINTER(C.c_uint64), i64]),
        "ntts_backbone_gemv_timeline": (C.c_int, [p, i32, i32, C.POINTER(C.c_uint64), i64, C.POINTER(i32)]),
        "ntts_codec_last_error": (C.c_char_p, [p]),
        "ntts_codec_create": (C.c_int, [C.POINTER(CodecConfigC), C.c_int, C.POINTER(p)]),
        "ntts_codec_destroy": (None, [p]),
        "ntts_codec_load_tensor": (C.c_int, [p, C.c_char_p, p, C.c_int, C.POINTER(i64), C.c_int, C.c_int]),
        "ntts_codec_finalize": (C.c_int, [p]),
        "ntts_codec_decode": (C.c_int, [p, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(f32), i64]),
        "ntts_codec_last_timing": (C.c_int, [p, C.POINTER(f32)]),
        "ntts_wav_out_len": (C.c_int, [C.POINTER(WavFormatC), i64, C.POINTER(i64)]),
        "ntts_codec_decode_fmt": (C.c_int, [p, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(WavFormatC), p, i64, C.POINTER(i32)]),
        "ntts_codec_decode_dev_fmt": (C.c_int, [p, i32, p, i32, C.POINTER(i32), p, i64, i32, p, C.POINTER(WavFormatC), C.POINTER(i32)]),
        "ntts_codec_convert": (C.c_int, [p, i32, C.POINTER(f32), i64, C.POINTER(i32), C.POINTER(WavFormatC), p, i64, C.POINTER(i32)]),
        "ntts_wav_stretch_len": (C.c_int, [i32, i64, C.POINTER(i64)]),
        "ntts_codec_stretch": (C.c_int, [p, i32, C.POINTER(f32), i64, C.POINTER(i32), C.POINTER(i32), C.POINTER(WavFormatC), p, i64, C.POINTER(i32),
                                         C.POINTER(i32), i64]),
        "ntts_codec_decode_speed": (C.c_int, [p, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(WavFormatC), p, i64, C.POINTER(i32)]),
        "ntts_codec_decode_dev_speed": (C.c_int, [p, i32, p, i32, C.POINTER(i32), C.POINTER(i32), p, i64, i32, p, C.POINTER(WavFormatC),
                                                  C.POINTER(i32)]),
        "ntts_codec_last_stretch_timing": (C.c_int, [p, C.POINTER(f32), C.POINTER(f32)]),
        "ntts_codec_normalize": (C.c_int, [p, i32, C.POINTER(f32), i64, C.POINTER(i32), C.POINTER(WavLoudnessC), C.POINTER(WavFormatC), p, i64,
                                           C.POINTER(i32), C.POINTER(C.c_double)]),
        "ntts_codec_measure_loudness": (C.c_int, [p, i32, C.POINTER(f32), i64, C.POINTER(i32), C.POINTER(C.c_double)]),
        "ntts_codec_decode_loud": (C.c_int, [p, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(WavLoudnessC), C.POINTER(WavFormatC), p,
                                             i64, C.POINTER(i32)]),
        "ntts_codec_decode_dev_loud": (C.c_int, [p, i32, p, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(WavLoudnessC), p, i64, i32, p,
                                                 C.POINTER(WavFormatC), C.POINTER(i32)]),
        "ntts_codec_last_loudness_timing": (C.c_int, [p, C.POINTER(f32), C.POINTER(f32)]),
        "ntts_wav_stream_create": (C.c_int, [p, C.POINTER(WavFormatC), i32, i32, C.POINTER(p)]),
        "ntts_wav_stream_destroy": (None, [p]),
        "ntts_wav_stream_last_error": (C.c_char_p, [p]),
        "ntts_wav_stream_push": (C.c_int, [p, i32, C.POINTER(i32), C.POINTER(f32), i64, C.POINTER(i32), C.POINTER(i32), p, i64, C.POINTER(i32)]),
        "ntts_wav_stream_count": (C.c_int, [C.POINTER(WavFormatC), i64, i32, C.POINTER(i64)]),
        "ntts_speed_stream_create": (C.c_int, [p, C.POINTER(WavFormatC), i32, i32, C.POINTER(p)]),
        "ntts_speed_stream_destroy": (None, [p]),
        "ntts_speed_stream_last_error": (C.c_char_p, [p]),
        "ntts_speed_stream_push": (C.c_int, [p, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(f32), i64, C.POINTER(i32), C.POINTER(i32), p, i64,
                                             C.POINTER(i32), C.POINTER(i32), i64, C.POINTER(i32)]),
        "ntts_speed_stream_count": (C.c_int, [i32, i64, i32, C.POINTER(i64)]),
        "ntts_streams_set_speed": (C.c_int, [p, C.POINTER(i32)]),
        "ntts_streams_set_format": (C.c_int, [p, C.POINTER(WavFormatC)]),
        "ntts_streams_pump_end_fmt": (C.c_int, [p, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(p),
                                                C.POINTER(i64), C.POINTER(i32), C.POINTER(i32)]),
        "ntts_encoder_last_error": (C.c_char_p, [p]),
        "ntts_encoder_create": (C.c_int, [C.POINTER(EncoderConfigC), C.c_int, C.POINTER(p)]),
        "ntts_encoder_destroy": (None, [p]),
        "ntts_encoder_load_tensor": (C.c_int, [p, C.c_char_p, p, C.c_int, C.POINTER(i64), C.c_int, C.c_int]),
        "ntts_encoder_finalize": (C.c_int, [p]),
        "ntts_encoder_encode": (C.c_int, [p, C.POINTER(f32), i64, C.POINTER(i32), i32, C.POINTER(i32)]),
        "ntts_encoder_read_stage": (C.c_int, [p, i32, C.POINTER(f32), i64, C.POINTER(i32), C.POINTER(i32)]),
        "ntts_encoder_last_timing": (C.c_int, [p, C.POINTER(f32)]),
        "ntts_host_alloc": (C.c_int, [C.c_size_t, C.POINTER(p)]),
        "ntts_host_free": (C.c_int, [p]),
        "ntts_stream_create": (C.c_int, [i32, C.POINTER(p)]),
        "ntts_stream_destroy": (C.c_int, [i32, p]),
        "ntts_k_gemm_bf16": (C.c_int, [p, i64, p, p, p, i64, i32, i32, i32, i32]),
        "ntts_k_gemm_probe": (C.c_int, [i32, i32, i32, i32, i32, i32, i32, C.POINTER(C.c_double)]),
        "ntts_k_rmsnorm_bf16": (C.c_int, [p, p, p, i32, i32, f32]),
        "ntts_k_fp8_quantize": (C.c_int, [p, p, i64, f32]),
        "ntts_k_gemm_fp8": (C.c_int, [p, p, p, f32, p, p, i32, i32, i32, i32]),
        "ntts_k_membw": (C.c_int, [C.c_size_t, i32, C.POINTER(C.c_double)]),
        "ntts_k_mfma_probe": (C.c_int, [p]),
        "ntts_k_silu_probe": (C.c_int, [p, p, i64, i32]),
        "ntts_k_launch_chain_probe": (C.c_int, [i32, i32, i32, i32, C.POINTER(C.c_double)]),
        "ntts_k_sample_probe": (C.c_int, [p, i64, i32, i32, i32, C.POINTER(i32), C.POINTER(f32), C.POINTER(f32), C.POINTER(f32),
                                          C.POINTER(C.c_uint64), i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
        "ntts_k_sample_full_probe": (C.c_int, [p, i64, i32, i32, i32, C.POINTER(f32), C.POINTER(f32), C.POINTER(f32), C.POINTER(C.c_uint64), i32,
                                               C.POINTER(i32), C.POINTER(i32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
        "ntts_k_head_penalty_probe": (C.c_int, [p, p, i32, i32, i32, i32, i32, f32, C.POINTER(C.c_uint32), C.POINTER(f32), C.POINTER(i32),
                                                C.POINTER(f32), C.POINTER(C.c_uint16), C.POINTER(f32), C.POINTER(i32), i32, C.POINTER(i32),
                                                C.POINTER(i32)]),
        "ntts_k_head_logprob_probe": (C.c_int, [p, p, i32, i32, i32, i32, i32, f32, C.POINTER(C.c_uint32), C.POINTER(f32), C.POINTER(i32),
                                                C.POINTER(f32), C.POINTER(C.c_uint16), C.POINTER(f32), C.POINTER(i32), C.POINTER(f32), i32,
                                                C.POINTER(i32), C.POINTER(i32), C.POINTER(f32)]),
        "ntts_k_head_score_probe": (C.c_int, [p, p, i32, i32, i32, i32, i32, f32, C.POINTER(i32), C.POINTER(f32), C.POINTER(f32), C.POINTER(i32),
                                              C.POINTER(f32), i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(f32), C.POINTER(f32), C.POINTER(i32),
                                              C.POINTER(f32)]),
        "ntts_k_attn_decode_form": (C.c_int, [i32, i32, i32, i32, i32]),
        "ntts_k_attn_decode_probe": (C.c_int, [p, i64, p, f32, p, p, i32, p, i32, p, p, i32, i32, i32, i32, i32, i32, i32, i32, p]),
        "ntts_k_attn_prefill_probe": (C.c_int, [p, i64, p, f32, p, p, i32, p, i32, i32, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32),
                                                i32, i32, i32, p, p, i32, p, p, f32, i32, i32, i32]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)  # AttributeError here == header/library drift: fail loudly
        fn.restype = res
        fn.argtypes = args
    _LIBS[path] = lib
    return lib


def _tensor_ptr(t):
    """(pointer, dtype code, shape, is_device, keepalive) for numpy fp32 / torch fp32|bf16 (cpu|cuda)."""
    if isinstance(t, np.ndarray):
        a = np.ascontiguousarray(t, dtype=np.float32)
        return a.ctypes.data, NTTS_DT_F32, a.shape, 0, a
    import torch  # plumbing only: tensor containers
    if isinstance(t, torch.Tensor):
        tt = t.detach().contiguous()
        if tt.dtype == getattr(torch, "float8_e4m3fn", None):      # a pre-quantised matrix of an fp8 checkpoint: its bytes
            return tt.data_ptr(), NTTS_DT_FP8_E4M3, tuple(tt.shape), int(tt.is_cuda), tt
        if tt.dtype == torch.bfloat16:
            code = NTTS_DT_BF16
        else:
            tt = tt.to(torch.float32)
            code = NTTS_DT_F32
        return tt.data_ptr(), code, tuple(tt.shape), int(tt.is_cuda), tt
    raise TypeError(f"unsupported tensor type {type(t)}")


# ---- the codec's output stage (include/neutts_hip.h ntts_wav_format): resample 24 kHz -> WAV_RATES, encode as float32 / PCM16 / G.711 mu-law
NATIVE_SAMPLE_RATE = 24000
WAV_RATES = (8000, 16000, 22050, 24000, 32000, 44100, 48000)
WAV_ENCODINGS = {"f32": (0, np.float32), "pcm16": (1, np.int16), "mulaw": (2, np.uint8)}
WAV_MAX_FILTER_WIDTH = 64


def wav_format(sample_rate=None, encoding="f32", filter_width=None, who: str = ""):
    """Checked (WavFormatC, numpy dtype, is_native) of an output format; None = 24 000 Hz / "f32" / width 6.  ValueError names the bad value."""
    rate = NATIVE_SAMPLE_RATE if sample_rate is None else sample_rate
    if isinstance(rate, (bool, np.bool_)) or not isinstance(rate, (int, np.integer)) or int(rate) not in WAV_RATES:
        raise ValueError(f"{who}sample_rate must be one of {WAV_RATES} (got {sample_rate!r})")
    enc = "f32" if encoding is None else encoding
    if not isinstance(enc, str) or enc not in WAV_ENCODINGS:
        raise ValueError(f"{who}encoding must be one of {tuple(WAV_ENCODINGS)} (got {encoding!r})")
    w = 6 if filter_width is None else filter_width
    if isinstance(w, (bool, np.bool_)) or not isinstance(w, (int, np.integer)) or not 1 <= w <= WAV_MAX_FILTER_WIDTH:
        raise ValueError(f"{who}filter_width must be an integer in [1, {WAV_MAX_FILTER_WIDTH}] (got {filter_width!r})")
    code, dtype = WAV_ENCODINGS[enc]
    return WavFormatC(int(rate), code, int(w)), dtype, (int(rate) == NATIVE_SAMPLE_RATE and enc == "f32")


def wav_out_len(n_in: int, sample_rate=None) -> int:
    """Samples at `sample_rate` of n_in samples at 24 kHz: ceil(n_in * rate / 24000) (ntts_wav_out_len's arithmetic)."""
    rate = int(wav_format(sample_rate)[0].sample_rate)
    return -(-int(n_in) * rate // NATIVE_SAMPLE_RATE)


# ---- speed: the pitch-preserving time stretch between the codec pass and the output stage (include/neutts_hip.h ntts_codec_stretch)
SPEED_PERMILLE_MIN, SPEED_PERMILLE_MAX = 500, 2000
STRETCH_HOP = 360


def speed_permille(speed, n: int, who: str = "") -> Optional[np.ndarray]:
    """Checked speeds of n utterances, one value or one per utterance, as the engine's integers per mille (round(speed * 1000)) -- int32 [n], or
    None when every utterance runs at 1.0 (None included): the calls of an engine without the stage.  ValueError names the bad value."""
    if speed is None:
        return None
    vals = list(speed) if isinstance(speed, (list, tuple, np.ndarray)) else [speed] * n
    if len(vals) != n:
        raise ValueError(f"{who}speed: {len(vals)} values for {n} utterances")
    pm = np.zeros(n, dtype=np.int32)
    for i, v in enumerate(vals):
        ok = not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, float, np.integer, np.floating)) and np.isfinite(v)
        if not ok or not SPEED_PERMILLE_MIN <= int(round(float(v) * 1000)) <= SPEED_PERMILLE_MAX:
            raise ValueError(f"{who}speed must be a number in [0.5, 2.0] (got {v!r})")
        pm[i] = int(round(float(v) * 1000))
    return None if (pm == 1000).all() else pm


def wav_stretch_len(n_in: int, permille: int) -> int:
    """Samples of n_in samples at a speed per mille: ceil(n_in * 1000 / permille) (ntts_wav_stretch_len's arithmetic)."""
    return -(-int(n_in) * 1000 // int(permille))


# ---- loudness: BS.1770 loudness normalisation between the time stretch and the output stage (include/neutts_hip.h ntts_codec_normalize)
LOUDNESS_TARGET_RANGE, LOUDNESS_PEAK_RANGE, LOUDNESS_MAX_GAIN_RANGE = (-70.0, 0.0), (-20.0, 0.0), (0.0, 60.0)
LOUDNESS_PEAK_DEFAULT, LOUDNESS_MAX_GAIN_DEFAULT = -1.0, 20.0


def _loudness_number(v, lo: float, hi: float, what: str, unit: str) -> float:
    ok = not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, float, np.integer, np.floating)) and np.isfinite(v)
    if not ok or not lo <= float(v) <= hi:
        raise ValueError(f"{what} must be a number in [{lo:g}, {hi:g}] {unit} (got {v!r})")
    return float(v)


def loudness_params(loudness, peak=LOUDNESS_PEAK_DEFAULT, max_gain=LOUDNESS_MAX_GAIN_DEFAULT, n: int = 1, who: str = ""):
    """Checked loudness settings of n utterances as the engine's ntts_wav_loudness array, or None when no utterance has the option on.  loudness:
    the target in LUFS, one value or one per utterance; None (or a None entry) = off.  peak (the sample-peak ceiling in dBFS) and max_gain (dB) are
    one value for the call.  ValueError names the bad value."""
    if loudness is None:
        return None
    vals = list(loudness) if isinstance(loudness, (list, tuple, np.ndarray)) else [loudness] * n
    if len(vals) != n:
        raise ValueError(f"{who}loudness: {len(vals)} values for {n} utterances")
    if all(v is None for v in vals):
        return None
    peak = _loudness_number(peak, *LOUDNESS_PEAK_RANGE, f"{who}loudness_peak", "dBFS")
    max_gain = _loudness_number(max_gain, *LOUDNESS_MAX_GAIN_RANGE, f"{who}loudness_max_gain", "dB")
    arr = (WavLoudnessC * n)()
    for i, v in enumerate(vals):
        if v is None:
            arr[i] = WavLoudnessC(0, 0.0, 0.0, 0.0)
        else:
            arr[i] = WavLoudnessC(1, _loudness_number(v, *LOUDNESS_TARGET_RANGE, f"{who}loudness", "LUFS"), peak, max_gain)
    return arr


def _loudness_rows(arr, rows):
    """The entries `rows` of an ntts_wav_loudness array, as a new array."""
    sub = (WavLoudnessC * len(rows))()
    for k, j in enumerate(rows):
        sub[k] = arr[j]
    return sub


@dataclass
class Sampling:
    """Keyword arguments of the reference's generate() call (ref:neutts/neutts.py:338-347), plus generate()'s own top_p / min_p (off -- 1.0 / 0.0 --
    in that call): TopPLogitsWarper / MinPLogitsWarper behind top-k, in transformers' order (include/neutts_hip.h: ntts_sampling).
    repetition_penalty / prompt_ignore_length (ABI 11): generate()'s `repetition_penalty` (1.0 = off, the reference's value) and
    RepetitionPenaltyLogitsProcessor's `prompt_ignore_length`; the penalty applies to greedy and sampled requests alike.
    top_k = TOP_K_OFF (-1): no top-k cut -- temperature, top_p and min_p act on the whole vocabulary (transformers' top_k=0 / None)."""
    max_length: int = 2048
    min_new_tokens: int = 50
    eos_token_id: int = 0
    do_sample: bool = True
    top_k: int = 50
    temperature: float = 1.0
    seed: int = 0
    top_p: float = 1.0
    min_p: float = 0.0
    repetition_penalty: float = 1.0
    prompt_ignore_length: int = 0

    def to_c(self) -> SamplingC:
        return SamplingC(self.max_length, self.min_new_tokens, self.eos_token_id, int(self.do_sample), self.top_k,
                         self.temperature, self.seed, self.top_p, self.min_p, self.repetition_penalty, self.prompt_ignore_length)


SAMPLE_CAP = 512                 # candidates the device sampler keeps (csrc/kernels/sample.h kSampleCap)
TOP_K_OFF = -1                   # Sampling.top_k: no top-k cut, sample over the whole vocabulary (include/neutts_hip.h NTTS_TOP_K_OFF)


def sample_probe(lib, logits_ptr: int, ld_logits: int, rows: int, vocab: int, group_width: int, top_k, temperature, top_p, min_p, seed,
                 step: int):
    """ntts_k_sample_probe: the engine's token choice on `rows` DEVICE bf16 logits rows at `logits_ptr` (row stride ld_logits elements); the
    sampling parameters are per row (scalars are broadcast).  group_width 0 = the full-row path, else the grouped path over groups of that
    many columns.  Returns (tokens [rows], [survivor ids of each row, in token-id order])."""
    def arr(v, dt):
        return np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=dt), (rows,)))
    k, t, tp, mp, sd = arr(top_k, np.int32), arr(temperature, np.float32), arr(top_p, np.float32), arr(min_p, np.float32), arr(seed, np.uint64)
    tok = np.zeros(rows, dtype=np.int32)
    n = np.zeros(rows, dtype=np.int32)
    ids = np.zeros((rows, SAMPLE_CAP), dtype=np.int32)
    i32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    rc = lib.ntts_k_sample_probe(C.c_void_p(logits_ptr), ld_logits, rows, vocab, group_width, k.ctypes.data_as(i32p), t.ctypes.data_as(f32p),
                                 tp.ctypes.data_as(f32p), mp.ctypes.data_as(f32p), sd.ctypes.data_as(C.POINTER(C.c_uint64)), step,
                                 tok.ctypes.data_as(i32p), n.ctypes.data_as(i32p), ids.ctypes.data_as(i32p))
    if rc != 0:
        raise NeuTTSHipError(rc, "ntts_k_sample_probe")
    return tok, [ids[r, : n[r]].copy() for r in range(rows)]


def sample_full_probe(lib, logits_ptr: int, ld_logits: int, rows: int, vocab: int, group_width: int, temperature, top_p, min_p, seed, step: int):
    """ntts_k_sample_full_probe: the engine's whole-vocabulary token choice (top_k = TOP_K_OFF) on `rows` DEVICE bf16 logits rows; parameters per
    row (scalars are broadcast).  group_width 0: the row's maximum from a pass over the row, else from the maxima of groups of that many columns
    (the results do not depend on it).  Returns (tokens [rows], survivor counts [rows], survivor bitmaps uint32 [rows][(vocab + 31) // 32] --
    bit c & 31 of word c >> 5 --, total integer masses uint64 [rows])."""
    def arr(v, dt):
        return np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=dt), (rows,)))
    t, tp, mp, sd = arr(temperature, np.float32), arr(top_p, np.float32), arr(min_p, np.float32), arr(seed, np.uint64)
    tok = np.zeros(rows, dtype=np.int32)
    n = np.zeros(rows, dtype=np.int32)
    keep = np.zeros((rows, (vocab + 31) // 32), dtype=np.uint32)
    total = np.zeros(rows, dtype=np.uint64)
    i32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    rc = lib.ntts_k_sample_full_probe(C.c_void_p(logits_ptr), ld_logits, rows, vocab, group_width, t.ctypes.data_as(f32p), tp.ctypes.data_as(f32p),
                                      mp.ctypes.data_as(f32p), sd.ctypes.data_as(C.POINTER(C.c_uint64)), step, tok.ctypes.data_as(i32p),
                                      n.ctypes.data_as(i32p), keep.ctypes.data_as(C.POINTER(C.c_uint32)), total.ctypes.data_as(C.POINTER(C.c_uint64)))
    if rc != 0:
        raise NeuTTSHipError(rc, "ntts_k_sample_full_probe")
    return tok, n, keep, total


HEAD_VARIANTS = {"64x64": 0, "128x128": 1, "256x256": 2, "256x288": 4, "gemv": 8}     # ntts_k_head_penalty_probe `variant`


def head_penalty_probe(lib, x_ptr: int, w_ptr: int, M: int, N: int, K: int, variant: int, seen=None, rep_pen=None, mask_eos=None,
                       fp8: bool = False, xscale: float = 1.0, _lse: bool = False):
    """ntts_k_head_penalty_probe: the engine's lm_head launch of tile `variant` (HEAD_VARIANTS) on DEVICE bf16 X [M][K] and W [N][K] (row-major; the
    probe packs W as the engine packs the head).  seen: None (the plain lm_head) or a bool / 0-1 array [M][N] of seen columns; rep_pen: [M]
    penalties; mask_eos: [M] column + 1 to mask, 0 = none.  Returns (logits fp32 [M][N], bf16 row bit patterns uint16 [M][N],
    partial maxima [M][n_part], their indices, columns per partial)."""
    words = None
    pen = None
    if seen is not None:
        bits = np.zeros((M, (N + 31) // 32 * 32), dtype=np.uint8)
        bits[:, :N] = np.asarray(seen, dtype=bool).reshape(M, N)
        words = np.ascontiguousarray(np.packbits(bits, axis=1, bitorder="little").view("<u4"))
        pen = np.ascontiguousarray(np.broadcast_to(np.asarray(rep_pen, dtype=np.float32), (M,)))
    me = None if mask_eos is None else np.ascontiguousarray(np.broadcast_to(np.asarray(mask_eos, dtype=np.int32), (M,)))
    cap = N // 16 + 16
    logits = np.zeros((M, N), dtype=np.float32)
    row16 = np.zeros((M, N), dtype=np.uint16)
    pv = np.zeros((M, cap), dtype=np.float32)
    pi = np.zeros((M, cap), dtype=np.int32)
    n_part, width = C.c_int32(), C.c_int32()
    i32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    head = (C.c_void_p(x_ptr), C.c_void_p(w_ptr), M, N, K, variant, int(fp8), xscale,
            None if words is None else words.ctypes.data_as(C.POINTER(C.c_uint32)),
            None if pen is None else pen.ctypes.data_as(f32p), None if me is None else me.ctypes.data_as(i32p),
            logits.ctypes.data_as(f32p), row16.ctypes.data_as(C.POINTER(C.c_uint16)), pv.ctypes.data_as(f32p), pi.ctypes.data_as(i32p))
    if _lse:
        ps = np.zeros((M, cap), dtype=np.float32)
        row_lse = np.zeros((M, 2), dtype=np.float32)
        rc = lib.ntts_k_head_logprob_probe(*head, ps.ctypes.data_as(f32p), cap, C.byref(n_part), C.byref(width), row_lse.ctypes.data_as(f32p))
    else:
        rc = lib.ntts_k_head_penalty_probe(*head, cap, C.byref(n_part), C.byref(width))
    if rc != 0:
        raise NeuTTSHipError(rc, "ntts_k_head_logprob_probe" if _lse else "ntts_k_head_penalty_probe")
    n = n_part.value
    # (the library wrote rows of n_part entries back to back)
    out = (logits, row16, pv.reshape(-1)[: M * n].reshape(M, n).copy(), pi.reshape(-1)[: M * n].reshape(M, n).copy(), width.value)
    if _lse:
        out += (ps.reshape(-1)[: M * n].reshape(M, n).copy(), row_lse[:, 0].copy(), row_lse[:, 1].copy())
    return out


def head_logprob_probe(lib, x_ptr: int, w_ptr: int, M: int, N: int, K: int, variant: int, seen=None, rep_pen=None, mask_eos=None,
                       fp8: bool = False, xscale: float = 1.0):
    """ntts_k_head_logprob_probe: head_penalty_probe's launch with the log-sum-exp epilogue (the lm_head kernels of an engine whose set_logprobs is on).
    Returns head_penalty_probe's five values, then part_sum [M][n_part] (sum over the partial's columns of exp(v - its maximum); 0 where that is -inf)
    and per row M (the row maximum) and log S as the sampling kernel's own merge computes them: logsumexp(row) = M + log S."""
    return head_penalty_probe(lib, x_ptr, w_ptr, M, N, K, variant, seen, rep_pen, mask_eos, fp8, xscale, _lse=True)


def head_score_probe(lib, x_ptr: int, w_ptr: int, M: int, N: int, K: int, variant: int, target, fp8: bool = False, xscale: float = 1.0):
    """ntts_k_head_score_probe: the scoring launch (the lm_head tile `variant` with the target-capture epilogue, then the merge kernel) on DEVICE bf16
    X [M][K] and W [N][K]; target: [M] columns in [0, N).  Returns a dict: logits fp32 [M][N], part_val / part_idx / part_sum [M][n_part], width
    (columns per partial), target_val [M], and the merged logprob / argmax / argmax_logprob [M].  The last four start as NaN (argmax: -1) on the device."""
    tg = np.ascontiguousarray(target, dtype=np.int32).reshape(M)
    cap = N // 16 + 16
    logits = np.zeros((M, N), dtype=np.float32)
    pv, ps = np.zeros((M, cap), dtype=np.float32), np.zeros((M, cap), dtype=np.float32)
    pi = np.zeros((M, cap), dtype=np.int32)
    tv, lp, alp = (np.zeros(M, dtype=np.float32) for _ in range(3))
    am = np.zeros(M, dtype=np.int32)
    n_part, width = C.c_int32(), C.c_int32()
    i32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    rc = lib.ntts_k_head_score_probe(C.c_void_p(x_ptr), C.c_void_p(w_ptr), M, N, K, variant, int(fp8), xscale, tg.ctypes.data_as(i32p),
                                     logits.ctypes.data_as(f32p), pv.ctypes.data_as(f32p), pi.ctypes.data_as(i32p), ps.ctypes.data_as(f32p), cap,
                                     C.byref(n_part), C.byref(width), tv.ctypes.data_as(f32p), lp.ctypes.data_as(f32p), am.ctypes.data_as(i32p),
                                     alp.ctypes.data_as(f32p))
    if rc != 0:
        raise NeuTTSHipError(rc, "ntts_k_head_score_probe")
    n = n_part.value
    cut = lambda a: a.reshape(-1)[: M * n].reshape(M, n).copy()     # (the library wrote rows of n_part entries back to back)
    return dict(logits=logits, part_val=cut(pv), part_idx=cut(pi), part_sum=cut(ps), width=width.value, target_val=tv, logprob=lp, argmax=am,
                argmax_logprob=alp)


class BackboneEngine:
    """One engine per GPU (per process): weights + paged KV + `max_batch` decode slots."""

    def __init__(self, cfg: dict, device: int = 0, lib_path: Optional[str] = None):
        self.lib = load_library(lib_path)
        if self.lib.ntts_abi_version() != ABI_VERSION:
            raise RuntimeError(f"libneutts_hip ABI mismatch: library {self.lib.ntts_abi_version()}, binding {ABI_VERSION} (rebuild: python neutts-air_amd/build.py)")
        self.cfg = dict(cfg)
        self._device, self._lib_path = device, lib_path
        c = BackboneConfigC(cfg["vocab_size"], cfg["hidden_size"], cfg["intermediate_size"], cfg["num_layers"],
                            cfg["num_heads"], cfg["num_kv_heads"], cfg.get("head_dim", 64), cfg.get("rms_eps", 1e-6),
                            cfg.get("max_context", 2048), cfg.get("max_batch", 1) + int(cfg.get("park_slots", 0)), cfg.get("num_pages", 0),
                            cfg.get("max_prefill_tokens", 0), int(cfg.get("tie_word_embeddings", True)),
                            int(cfg.get("attention_bias", True)), int(cfg.get("qk_norm", False)),
                            {"bf16": NTTS_W_BF16, "fp8": NTTS_W_FP8_E4M3, "fp8_e4m3": NTTS_W_FP8_E4M3}[str(cfg.get("weight_dtype", "bf16"))],
                            int(cfg.get("park_slots", 0)))
        self.fp8 = c.weight_dtype == NTTS_W_FP8_E4M3
        h = C.c_void_p()
        rc = self.lib.ntts_backbone_create(C.byref(c), device, C.byref(h))
        if rc != 0:
            raise NeuTTSHipError(rc, (self.lib.ntts_last_error(None) or b"").decode())
        self.h = h
        # cfg["park_slots"] = P extra PARKING rows behind the cfg["max_batch"] decode slots (ABI 9 ntts_backbone_config.park_slots: the library counts
        # them into its max_batch): rows max_batch .. max_batch + P - 1 take prompt passes but never decode; activate() moves one into a decode slot
        self.park_slots = c.park_slots
        self.n_rows = c.max_batch                         # every slot, parking rows included (the library's max_batch)
        self.max_batch = c.max_batch - c.park_slots       # decode slots (rows of the decode step)
        self._free_park: List[int] = list(range(self.n_rows - 1, self.max_batch - 1, -1))
        self.max_context = c.max_context
        self.vocab_size = c.vocab_size
        self._free: List[int] = list(range(self.max_batch - 1, -1, -1))   # host-side pool of decode slots (pop -> slot 0 first)
        self.counters = {"decode_steps": 0, "prefill_calls": 0, "prefill_prompts": 0, "prefill_tokens": 0}   # diagnostics (bench.py)
        self.logprobs = False                             # set_logprobs

    # -- decode-slot pool: every path that admits a request (generate, the streaming generators) draws from here, so an
    #    unfinished stream and a later call can never be handed the same slot
    def acquire_slot(self) -> int:
        if not self._free:
            raise NeuTTSHipError(-4, f"all {self.max_batch} decode slots are in use")
        return self._free.pop()

    def free_slots(self) -> int:
        return len(self._free)

    # -- plumbing
    def _chk(self, rc: int):
        if rc != 0:
            raise NeuTTSHipError(rc, (self.lib.ntts_last_error(self.h) or b"").decode())

    def close(self):
        if getattr(self, "h", None):
            self.lib.ntts_backbone_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- weights
    def load_tensor(self, name: str, t):
        ptr, code, shape, is_dev, keep = _tensor_ptr(t)
        shp = (C.c_int64 * len(shape))(*shape)
        self._chk(self.lib.ntts_backbone_load_tensor(self.h, name.encode(), C.c_void_p(ptr), code, shp, len(shape), is_dev))
        del keep

    def load_state_dict(self, sd: Dict[str, object], inv_freq=None, input_scales: Optional[Dict[str, float]] = None):
        """HF Qwen2ForCausalLM state dict (+ rope.inv_freq; computed like hf:...modeling_qwen2.py:86 if absent).
        fp8 engines (weight_dtype="fp8"): bf16 / fp32 matrices are quantised on upload; matrices that are ALREADY torch.float8_e4m3fn
        (a pre-quantised checkpoint) are stored as they are and need their `<module>.weight_scale` entry; the static activation scales
        come as `*.input_scale` entries of `sd` (static-fp8 checkpoints) or as the `input_scales` dict {tensor name: float}."""
        for k, v in sd.items():
            if k.endswith("rotary_emb.inv_freq"):
                continue
            if k.endswith(".input_scale"):
                v = np.asarray(v.float().cpu() if hasattr(v, "cpu") else v, dtype=np.float32).reshape(1)
            elif k.endswith(".weight_scale"):       # pre-quantised fp8 checkpoint: per-output-channel (or per-matrix) scales, fp32 on the way in
                v = np.ascontiguousarray(np.asarray(v.float().cpu() if hasattr(v, "cpu") else v, dtype=np.float32))
            self.load_tensor(k, v)
        for k, v in (input_scales or {}).items():
            self.load_tensor(k, np.asarray([v], dtype=np.float32))
        if inv_freq is None:
            raise ValueError("inv_freq (fp32 [head_dim/2]) must be supplied: it is a model buffer, not a constant")
        self.load_tensor("rope.inv_freq", np.asarray(inv_freq, dtype=np.float32))
        self._chk(self.lib.ntts_backbone_finalize(self.h))

    def arena(self):
        p, n = C.c_void_p(), C.c_size_t()
        self._chk(self.lib.ntts_backbone_arena(self.h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def arena_derived(self):
        """(offset, bytes) of the arena range a broadcast may skip (rebuilt by adopt_arena on the receiver)."""
        o, n = C.c_size_t(), C.c_size_t()
        self._chk(self.lib.ntts_backbone_arena_derived(self.h, C.byref(o), C.byref(n)))
        return o.value, n.value

    def arena_copy(self, buf_ptr: int, nbytes: int, to_arena: bool):
        self._chk(self.lib.ntts_backbone_arena_copy(self.h, C.c_void_p(buf_ptr), nbytes, int(to_arena)))

    KERNELS = ["attn_decode_kernel", "gemm_qkv", "gemm_o_proj_splitk", "gemm_gate_up_silu", "gemm_down_splitk",
               "gemm_lm_head_argmax", "add_rmsnorm_kernel"]

    def time_kernel(self, which: int, iters: int = 20):
        ms, nb, nl = C.c_float(), C.c_double(), C.c_int32()
        self._chk(self.lib.ntts_backbone_time_kernel(self.h, which, iters, C.byref(ms), C.byref(nb), C.byref(nl)))
        return ms.value, nb.value, nl.value

    def adopt_arena(self):
        self._chk(self.lib.ntts_backbone_adopt_arena(self.h))

    def twin(self, share: bool = True) -> "BackboneEngine":
        """A second engine with this one's configuration and weights -- its own KV pool, slot state, stream and step graph.  What
        running several batches at once needs: the twins' step graphs replayed alternately (each chain fills the other's launch gaps),
        one twin's prompt pass beside another's decode steps (bench.py static mode, EngineGang).  share=True: the twin READS THIS
        ENGINE'S ARENA (ntts_backbone_share_arena: no second copy of the weights; this engine is kept alive by the twin);
        share=False: its own arena, filled by one device-to-device copy."""
        self.sync()
        t = BackboneEngine(self.cfg, self._device, self._lib_path)
        if share:
            t._chk(self.lib.ntts_backbone_share_arena(t.h, self.h))
            t._donor = self
        else:
            ptr, nbytes = self.arena()
            t.arena_copy(ptr, nbytes, True)
            t.adopt_arena()
        if getattr(self, "logits_range", None):
            t.set_logits_range(*self.logits_range)          # (an opt-in restricted lm_head goes along: its own compacted copy)
        if self.logprobs:
            t.set_logprobs(True)                            # (the switch is per engine)
        return t

    # -- requests
    def prefill(self, prompts: Sequence[Sequence[int]], slots: Sequence[int], sampling: Sequence[Sampling],
                donors: Optional[Sequence[Optional[tuple]]] = None):
        """donors (optional): per prompt None or (donor_slot, shared_len) -- re-use the KV pages of the first
        `shared_len` tokens (rounded down to whole pages) of a running slot / an earlier prompt of this call whose
        prompt starts with the same tokens (include/neutts_hip.h: ntts_backbone_prefill_shared)."""
        n = len(prompts)
        lens = np.array([len(p) for p in prompts], dtype=np.int32)
        ids = np.ascontiguousarray(np.concatenate([np.asarray(p, dtype=np.int32) for p in prompts]))
        sl = np.asarray(slots, dtype=np.int32)
        try:
            self._prefill_call(n, ids, lens, sl, sampling, donors)
        except NeuTTSHipError:
            raise                      # the engine admitted nothing: slots drawn from the pool stay with the caller to release
        self._mark_busy(slots)
        self.counters["prefill_calls"] += 1
        self.counters["prefill_prompts"] += n
        self.counters["prefill_tokens"] += int(lens.sum())

    def _prefill_call(self, n, ids, lens, sl, sampling, donors):
        sc = (SamplingC * n)(*[s.to_c() for s in sampling])
        i32p = C.POINTER(C.c_int32)
        if donors is None or all(d is None for d in donors):
            self._chk(self.lib.ntts_backbone_prefill(self.h, n, ids.ctypes.data_as(i32p), lens.ctypes.data_as(i32p),
                                                     sl.ctypes.data_as(i32p), sc))
            return
        ds = np.array([-1 if d is None else d[0] for d in donors], dtype=np.int32)
        dl = np.array([0 if d is None else d[1] for d in donors], dtype=np.int32)
        self._chk(self.lib.ntts_backbone_prefill_shared(self.h, n, ids.ctypes.data_as(i32p), lens.ctypes.data_as(i32p),
                                                        sl.ctypes.data_as(i32p), sc, ds.ctypes.data_as(i32p),
                                                        dl.ctypes.data_as(i32p)))

    def kv_stats(self) -> dict:
        fp, tp, tc, ts = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64()
        self._chk(self.lib.ntts_backbone_kv_stats(self.h, C.byref(fp), C.byref(tp), C.byref(tc), C.byref(ts)))
        return {"free_pages": fp.value, "total_pages": tp.value, "prompt_tokens_computed": tc.value,
                "prompt_tokens_shared": ts.value}

    def decode(self, n_steps: int = 1):
        self._chk(self.lib.ntts_backbone_decode(self.h, n_steps))
        self.counters["decode_steps"] += n_steps

    def read(self, slot: int):
        out = np.empty(self.max_context, dtype=np.int32)
        n, fin = C.c_int32(), C.c_int32()
        self._chk(self.lib.ntts_backbone_read(self.h, slot, out.ctypes.data_as(C.POINTER(C.c_int32)), len(out),
                                              C.byref(n), C.byref(fin)))
        return out[: n.value].tolist(), bool(fin.value)

    def poll_begin(self):
        """Asynchronous poll: snapshot every slot's state / new-token count behind the work enqueued so far (no host wait)."""
        self._chk(self.lib.ntts_backbone_poll_begin(self.h))

    def poll_end(self):
        """(state, n_new) of the snapshot opened by poll_begin; waits for that copy only, not for work enqueued after it."""
        st = np.empty(self.n_rows, dtype=np.int32)
        nn = np.empty(self.n_rows, dtype=np.int32)
        i32p = C.POINTER(C.c_int32)
        self._chk(self.lib.ntts_backbone_poll_end(self.h, st.ctypes.data_as(i32p), nn.ctypes.data_as(i32p)))
        return st, nn

    def read_finished(self, slot: int) -> List[int]:
        """The ids of a slot the last completed snapshot showed finished -- copied past the decode steps still queued."""
        out = np.empty(self.max_context, dtype=np.int32)
        n = C.c_int32()
        self._chk(self.lib.ntts_backbone_read_finished(self.h, slot, out.ctypes.data_as(C.POINTER(C.c_int32)), len(out), C.byref(n)))
        return out[: n.value].tolist()

    def set_logprobs(self, enable: bool = True):
        """Per-token log-probabilities on / off for this engine (ntts_backbone_set_logprobs; include/neutts_hip.h has the definition): while on, every
        request records log softmax(processed logits row)[token] beside each id.  NTTS_ESTATE while a slot or parking row is in use."""
        self._chk(self.lib.ntts_backbone_set_logprobs(self.h, int(bool(enable))))
        self.logprobs = bool(enable)

    def read_logprobs(self, slot: int) -> np.ndarray:
        """The log-probabilities of the ids read(slot) returns, entry for entry (blocking).  NTTS_ESTATE while set_logprobs is off."""
        out = np.empty(self.max_context, dtype=np.float32)
        n = C.c_int32()
        self._chk(self.lib.ntts_backbone_read_logprobs(self.h, slot, out.ctypes.data_as(C.POINTER(C.c_float)), len(out), C.byref(n)))
        return out[: n.value].copy()

    def read_finished_logprobs(self, slot: int) -> np.ndarray:
        """read_logprobs for a slot the last completed snapshot showed finished -- copied past the decode steps still queued, like read_finished."""
        out = np.empty(self.max_context, dtype=np.float32)
        n = C.c_int32()
        self._chk(self.lib.ntts_backbone_read_finished_logprobs(self.h, slot, out.ctypes.data_as(C.POINTER(C.c_float)), len(out), C.byref(n)))
        return out[: n.value].copy()

    def score_call(self, seqs, slots: Sequence[int], score_from: Sequence[int], chunk_rows: int = 0):
        """One ntts_backbone_score call (include/neutts_hip.h has the definition): `seqs` on the FREE slots `slots`, sequence i scored from position
        score_from[i].  Blocking; the slots and their KV pages are free again on return.  Returns the packed (logprobs, argmax ids, argmax logprobs)."""
        lens = np.ascontiguousarray([len(q) for q in seqs], dtype=np.int32)
        ids = np.ascontiguousarray(np.concatenate([np.asarray(q, dtype=np.int64) for q in seqs]) if len(seqs) else [], dtype=np.int32)
        sl = np.ascontiguousarray(slots, dtype=np.int32)
        sf = np.ascontiguousarray(score_from, dtype=np.int32)
        if not (len(lens) == len(sl) == len(sf)):
            raise ValueError("score_call: one slot and one score_from per sequence")
        cap = int(max(0, int((lens.astype(np.int64) - sf).clip(min=0).sum())))
        lp, alp = np.empty(cap, dtype=np.float32), np.empty(cap, dtype=np.float32)
        am = np.empty(cap, dtype=np.int32)
        n = C.c_int64()
        i32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_float)
        self._chk(self.lib.ntts_backbone_score(self.h, len(lens), ids.ctypes.data_as(i32p), lens.ctypes.data_as(i32p), sl.ctypes.data_as(i32p),
                                               sf.ctypes.data_as(i32p), int(chunk_rows), lp.ctypes.data_as(f32p), am.ctypes.data_as(i32p),
                                               alp.ctypes.data_as(f32p), cap, C.byref(n)))
        return lp[: n.value], am[: n.value], alp[: n.value]

    def score(self, seqs, score_from=None, chunk_rows: int = 0):
        """Teacher-forced scoring of given token sequences: for each, the model's log-probability of tokens score_from .. len - 1 given the ones before
        (score_from: None = 1, an int for all, or one per sequence).  No logits processor enters; see include/neutts_hip.h.  The sequences are packed
        into as many calls as max_prefill_tokens and the free decode slots require; running requests are not touched, and a sequence's values are
        bit-identical for every chunk_rows and whichever sequences share its call (one lm_head tile per engine).  chunk_rows above 8192 or
        max_prefill_tokens is taken as the smaller of the two.  Returns one
        (logprobs float32, argmax_ids int32, argmax_logprobs float32) triple of numpy arrays per sequence, len - score_from entries each."""
        seqs = [list(q) for q in seqs]
        if score_from is None:
            sf = [1] * len(seqs)
        elif isinstance(score_from, (int, np.integer)):
            sf = [int(score_from)] * len(seqs)
        else:
            sf = [int(v) for v in score_from]
        if len(sf) != len(seqs):
            raise ValueError("score: one score_from per sequence")
        tmax = int(self.cfg.get("max_prefill_tokens", 0) or 16384)
        out = [None] * len(seqs)
        i = 0
        while i < len(seqs):
            if not self._free:
                raise NeuTTSHipError(-4, "score: no free decode slot")
            j, tok = i, 0
            while j < len(seqs) and j - i < len(self._free) and (j == i or tok + len(seqs[j]) <= tmax):
                tok += len(seqs[j])
                j += 1
            slots = self._free[-1: -(j - i) - 1: -1]          # borrowed for the call only: the library leaves them free
            lp, am, alp = self.score_call(seqs[i:j], slots, sf[i:j], chunk_rows)
            o = 0
            for k in range(i, j):
                m = len(seqs[k]) - sf[k]
                out[k] = (lp[o:o + m].copy(), am[o:o + m].copy(), alp[o:o + m].copy())
                o += m
            i = j
        return out

    def read_score_logits(self, row: int) -> np.ndarray:
        """Debug tap (set_debug(True) before the score call): the fp32 lm_head row behind output entry `row` of the most recent score_call."""
        out = np.empty(self.vocab_size, dtype=np.float32)
        self._chk(self.lib.ntts_backbone_read_score_logits(self.h, int(row), out.ctypes.data_as(C.POINTER(C.c_float)), len(out)))
        return out

    def read_all_array(self):
        """Every slot's new ids in one call, as arrays: (ids [max_batch, max_context] int32 -- row s valid up to n[s]),
        n [max_batch], finished [max_batch] bool).  The batch hand-off to the codec stays in numpy (no Python lists)."""
        out = np.empty((self.n_rows, self.max_context), dtype=np.int32)
        n = np.empty(self.n_rows, dtype=np.int32)
        fin = np.empty(self.n_rows, dtype=np.int32)
        i32p = C.POINTER(C.c_int32)
        self._chk(self.lib.ntts_backbone_read_all(self.h, out.ctypes.data_as(i32p), self.max_context,
                                                  n.ctypes.data_as(i32p), fin.ctypes.data_as(i32p)))
        return out, n, fin.astype(bool)

    def read_all(self):
        """Every slot's new ids in one call: ([ids per slot], [finished per slot])."""
        out, n, fin = self.read_all_array()
        return [out[s, : n[s]].tolist() for s in range(self.max_batch)], [bool(f) for f in fin]

    def poll(self):
        st = np.empty(self.n_rows, dtype=np.int32)
        nn = np.empty(self.n_rows, dtype=np.int32)
        i32p = C.POINTER(C.c_int32)
        self._chk(self.lib.ntts_backbone_poll(self.h, st.ctypes.data_as(i32p), nn.ctypes.data_as(i32p)))
        return st, nn

    def warm_up(self, decode_steps: int = 2):
        """One throw-away request through slot 0 (a 1-token prompt, `decode_steps` greedy steps): captures and instantiates the
        decode-step hipGraph and lets the HIP runtime size its command pools, so that the first real request does not pay for
        either.  Serving start-up hygiene; the engine must be finalised and slot 0 free."""
        eos = self.logits_range[2] if getattr(self, "logits_range", None) else 0      # (a restricted lm_head accepts its own EOS id only)
        sp = Sampling(max_length=2 + decode_steps, min_new_tokens=1 + decode_steps, eos_token_id=eos, do_sample=False)
        self.prefill([[1 % self.vocab_size]], [0], [sp])
        self.decode(decode_steps)
        self.sync()
        self.release(0)
        self.sync()
        # The runtime sizes its pools by the number of graph replays that were ever queued before a synchronisation: the first
        # call AFTER the first long decode call pays for it once (43 ms on the host, measured in bench.py's step walls).  With
        # `decode_steps` as long as a real decode call, a second throw-away prompt pass absorbs that too.
        if decode_steps > 8:
            self.prefill([[1 % self.vocab_size]], [0], [Sampling(max_length=3, min_new_tokens=1, eos_token_id=eos, do_sample=False)])
            self.sync()
            self.release(0)
            self.sync()

    def set_prefill_cu_mask(self, mask_words: Optional[Sequence[int]]):
        """Run this engine's prompt passes on a side stream restricted to the CUs of `mask_words` (32-bit words, bit i of word w =
        CU 32 w + i); None / empty = default.  See include/neutts_hip.h: ntts_backbone_set_prefill_cu_mask."""
        words = list(mask_words or [])
        arr = (C.c_uint32 * max(1, len(words)))(*words)
        self._chk(self.lib.ntts_backbone_set_prefill_cu_mask(self.h, arr, len(words)))

    def stream(self) -> int:
        st = C.c_void_p()
        self._chk(self.lib.ntts_backbone_stream(self.h, C.byref(st)))
        return st.value or 0

    def export_codes(self, slots: Sequence[int], speech_base: int, n_codes: int, codes_dev_ptr: int, stride: int,
                     lens_dev_ptr: int, modulo: bool = False):
        """Device-side id -> code hand-off (ntts_backbone_export_codes): codes land in a caller-owned DEVICE int32 buffer
        [len(slots), stride], their counts in a DEVICE int32 buffer [len(slots)]; asynchronous on the engine's stream."""
        sl = np.ascontiguousarray(slots, dtype=np.int32)
        self._chk(self.lib.ntts_backbone_export_codes(self.h, len(sl), sl.ctypes.data_as(C.POINTER(C.c_int32)), speech_base,
                                                      n_codes, int(modulo), C.c_void_p(codes_dev_ptr), stride,
                                                      C.c_void_p(lens_dev_ptr)))

    def release(self, slot: int):
        self._chk(self.lib.ntts_backbone_release(self.h, slot))
        pool = self._free if slot < self.max_batch else self._free_park
        if slot not in pool:
            pool.append(slot)

    def acquire_park(self) -> int:
        if not self._free_park:
            raise NeuTTSHipError(-4, f"all {self.park_slots} parking rows are in use")
        return self._free_park.pop()

    def activate(self, park_rows: Sequence[int], slots: Sequence[int]):
        """Parked requests -> free decode slots (ntts_backbone_activate): stream-ordered behind the prompt pass that filled the parking rows and
        ahead of the next decode step.  The caller holds the slots (acquire_slot) and gets the parking rows back."""
        a = np.ascontiguousarray(park_rows, dtype=np.int32)
        b = np.ascontiguousarray(slots, dtype=np.int32)
        self._chk(self.lib.ntts_backbone_activate(self.h, len(a), a.ctypes.data_as(C.POINTER(C.c_int32)), b.ctypes.data_as(C.POINTER(C.c_int32))))
        for r in a.tolist():
            if r not in self._free_park:
                self._free_park.append(r)

    def release_many(self, slots: Sequence[int]):
        """release() for a whole set of slots with one stream operation."""
        sl = np.ascontiguousarray(slots, dtype=np.int32)
        self._chk(self.lib.ntts_backbone_release_many(self.h, len(sl), sl.ctypes.data_as(C.POINTER(C.c_int32))))
        for s in sl.tolist():
            pool = self._free if s < self.max_batch else self._free_park
            if s not in pool:
                pool.append(s)

    def _mark_busy(self, slots: Sequence[int]):
        """Callers that choose slot numbers themselves (tests, bench): keep the pool consistent."""
        for s in slots:
            if s in self._free:
                self._free.remove(s)

    def sync(self):
        self._chk(self.lib.ntts_backbone_sync(self.h))

    def set_gang(self, chains: int):
        """PIN how many decode chains (engines of an EngineGang, itself included) the engine assumes side by side on the GPU: the decode
        step's GEMM tiles and XCD placement are chosen for that (ntts_backbone_set_gang).  0 = count them (the default since ABI 9: engines
        of the same arena that decoded within the last 50 ms); both shapes keep their captured step graph.  Tests, sweeps, profiling."""
        self._chk(self.lib.ntts_backbone_set_gang(self.h, int(chains)))

    def calibrate(self, enable: bool = True):
        """fp8 calibration mode of a BF16 engine (ntts_backbone_calibrate): the prompt passes that follow record max |x| of every GEMM input."""
        self._chk(self.lib.ntts_backbone_calibrate(self.h, int(bool(enable))))

    def fp8_input_scales(self, margin: float = 1.0) -> Dict[str, float]:
        """The static `input_scale`s of the fp8 model from the record so far: amax / 448 x margin, under the tensor names a static-fp8
        checkpoint uses (what load_state_dict(..., input_scales=...) of a weight_dtype='fp8' engine takes)."""
        L = int(self.cfg["num_layers"])
        a = np.zeros(4 * L + 1, dtype=np.float32)
        self._chk(self.lib.ntts_backbone_read_amax(self.h, a.ctypes.data_as(C.POINTER(C.c_float)), len(a)))
        if not (a > 0).all():
            raise NeuTTSHipError(-4, "calibration saw no data for some GEMM inputs: run prompt passes between calibrate() and fp8_input_scales()")
        out = {"lm_head.input_scale": float(a[4 * L]) / 448.0 * margin}
        for i in range(L):
            for j, t in enumerate(("self_attn.q_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.down_proj")):
                out[f"model.layers.{i}.{t}.input_scale"] = float(a[4 * i + j]) / 448.0 * margin
        return out

    def set_logits_range(self, lo: Optional[int], hi: int = 0, eos_id: int = 0):
        """OPT-IN: lm_head over the token ids [lo, hi) + eos_id only (ntts_backbone_set_logits_range; lo=None restores the full head).
        The reference takes its argmax / top-k over the whole vocabulary: identical ids only while its choice lies in the range."""
        if lo is None:
            self._chk(self.lib.ntts_backbone_set_logits_range(self.h, -1, 0, 0))
        else:
            self._chk(self.lib.ntts_backbone_set_logits_range(self.h, int(lo), int(hi), int(eos_id)))
        self.logits_range = None if lo is None else (int(lo), int(hi), int(eos_id))

    def set_stream(self, stream: Optional[int]):
        """Run the engine's work on the caller's HIP stream (a hipStream_t as an integer, e.g. torch.cuda.Stream().cuda_stream); None = its own."""
        self._chk(self.lib.ntts_backbone_set_stream(self.h, C.c_void_p(stream or None)))

    def set_prefill_stream(self, stream: Optional[int]):
        """Prompt passes on the caller's HIP stream, event-ordered with the engine's stream (ntts_backbone_set_prefill_stream);
        None = back on the engine's stream."""
        self._chk(self.lib.ntts_backbone_set_prefill_stream(self.h, C.c_void_p(stream or None)))

    def set_debug(self, keep_logits: bool):
        self._chk(self.lib.ntts_backbone_set_debug(self.h, int(keep_logits)))

    def read_logits(self, slot: int) -> np.ndarray:
        out = np.empty(self.vocab_size, dtype=np.float32)
        self._chk(self.lib.ntts_backbone_read_logits(self.h, slot, out.ctypes.data_as(C.POINTER(C.c_float)), len(out)))
        return out

    def read_seen(self, slot: int) -> np.ndarray:
        """The lm_head columns slot `slot`'s repetition penalty counts as seen (ntts_backbone_read_seen), as a sorted array of column indices:
        token ids, or with set_logits_range positions in [lo, hi) followed by the EOS column.  NTTS_ESTATE before the first penalised request."""
        words = np.zeros((self.vocab_size + 31) // 32, dtype=np.uint32)
        self._chk(self.lib.ntts_backbone_read_seen(self.h, slot, words.ctypes.data_as(C.POINTER(C.c_uint32)), len(words)))
        return np.flatnonzero(np.unpackbits(words.view(np.uint8), bitorder="little")[: self.vocab_size])

    def debug_force(self, slot: int, token: int):
        self._chk(self.lib.ntts_backbone_debug_force(self.h, slot, token))

    def last_timing(self):
        a, b = C.c_float(), C.c_float()
        self._chk(self.lib.ntts_backbone_last_timing(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def gemv_timeline(self, which: int, layer: int = 0) -> np.ndarray:
        """[workgroups, 16] phase timestamps (100 MHz ticks) of one small-batch GEMV launch: which = 2 o_proj, 3 gate/up, 4 down_proj."""
        out = np.zeros((4096, 16), dtype=np.uint64)
        n = C.c_int32()
        self._chk(self.lib.ntts_backbone_gemv_timeline(self.h, which, layer, out.ctypes.data_as(C.POINTER(C.c_uint64)), out.size, C.byref(n)))
        return out[: n.value]

    def attn_timeline(self, layer: int = 0) -> np.ndarray:
        """Phase timestamps of one decode-attention launch: [max_batch, kv_heads, 4 waves, 8 phases], 100 MHz ticks."""
        nkv = self.cfg["num_kv_heads"]
        out = np.zeros((self.max_batch, nkv, 4, 8), dtype=np.uint64)
        self._chk(self.lib.ntts_backbone_attn_timeline(self.h, layer, out.ctypes.data_as(C.POINTER(C.c_uint64)), out.size))
        return out

    def step_bytes(self) -> float:
        d = C.c_double()
        self._chk(self.lib.ntts_backbone_step_bytes(self.h, C.byref(d)))
        return d.value

    # -- continuous batching (host scheduler): keep every slot busy until all prompts are done
    def generate(self, prompts: Sequence[Sequence[int]], sampling, steps_per_poll: int = 16,
                 prefill_token_budget: Optional[int] = None, share_prefix: bool = False, min_admit: int = 1,
                 on_finished=None, run_ahead: bool = True, admit_gate=None, on_admit=None, return_logprobs: bool = False) -> List[List[int]]:
        """Batched equivalent of calling ref:neutts/neutts.py:338-351 once per prompt.
        Returns the NEW ids of each prompt (prompt stripped), in order.
        return_logprobs=True (needs set_logprobs(True)): returns (ids, logprobs) -- one float32 array per prompt, entry for entry beside its ids,
        read before the slot is released (also when on_finished is set).
        share_prefix=True: a prompt that starts like one already in flight (same speaker: chat header + reference
        text, ref:neutts/neutts.py:307,315-325) re-uses that slot's KV pages for the common whole pages.
        min_admit: waiting prompts are admitted only once that many slots are free (or nothing is running): a prompt pass over
        a handful of prompts runs the big GEMM tiles nearly empty, so under load it pays to let a few slots idle for some steps
        and prefill them together.
        run_ahead (default): the scheduler keeps ONE burst of `steps_per_poll` decode steps queued ahead of its own bookkeeping --
        it enqueues burst k + 1 and only then reads the slot states as they were after burst k (ntts_backbone_poll_begin / _end),
        so the GPU never idles while the host reads finished rows, releases slots and packs the next prompt pass.  The price is
        that a finished row is noticed up to one burst later (it is carried along masked meanwhile: stopping is decided on the
        device, the ids cannot differ).
        on_finished(request_index, slot, n_new): called for every finished request BEFORE its slot is released, INSTEAD of
        copying its ids to the host (that request's entry of the result is then []): the hook of a device-side hand-off
        (ntts_backbone_export_codes enqueued from it is ordered before the slot's re-use).
        admit_gate(n_free, n_wanted) -> bool replaces the `min_admit` test while requests are running (n_wanted = min(min_admit,
        requests waiting)); on_admit(n_prompts) is called after every prompt pass: the two hooks by which an EngineGang coordinates
        its engines' admissions (a prompt pass takes an engine's lane for ~ 0.8 us per prompt token; with nothing running the gate
        is not asked)."""
        it = self.generate_iter(prompts, sampling, steps_per_poll, prefill_token_budget, share_prefix, min_admit, on_finished, run_ahead,
                                admit_gate, on_admit, return_logprobs)
        while True:
            try:
                next(it)
            except StopIteration as done:
                return done.value

    def generate_iter(self, prompts: Sequence[Sequence[int]], sampling, steps_per_poll: int = 16,
                      prefill_token_budget: Optional[int] = None, share_prefix: bool = False, min_admit: int = 1,
                      on_finished=None, run_ahead: bool = True, admit_gate=None, on_admit=None, return_logprobs: bool = False):
        """generate() as a generator: yields (None) once per scheduler iteration -- after this engine's next burst and snapshot
        are enqueued -- and returns generate()'s result as the StopIteration value.  What EngineGang alternates between: while one
        engine's scheduler waits for its previous snapshot, the other engines' bursts are already queued on their own streams."""
        if isinstance(sampling, Sampling):
            sampling = [sampling] * len(prompts)
        if return_logprobs and not self.logprobs:
            raise NeuTTSHipError(-4, "return_logprobs: log-probabilities are not recorded, call set_logprobs(True) first")
        budget = prefill_token_budget or self.cfg.get("max_prefill_tokens", 0) or 16384
        # validate up front: a request that cannot run must not strand the ones admitted before it
        for i, (p, sp) in enumerate(zip(prompts, sampling)):
            if len(p) < 1:
                raise ValueError(f"prompt {i} is empty")
            if not (len(p) < sp.max_length <= self.max_context):
                raise ValueError(f"prompt {i}: need len(prompt) < max_length <= max_context "
                                 f"({len(p)}, {sp.max_length}, {self.max_context})")
            if len(p) > budget:
                raise ValueError(f"prompt {i}: {len(p)} tokens exceed max_prefill_tokens {budget}")
        # KV admission control: a request is admitted only if the pool can hold it up to ITS max_length next to everything
        # already running (pages are allocated as the sequence grows; without the reservation two admitted requests could
        # starve each other in the middle of decoding)
        # Pages held OUTSIDE this call (a suspended infer_stream generator, slots another caller prefilled) are not this scheduler's
        # to hand out: the reservation budget is what was free when the call started (comparing with the pool's size let
        # the scheduler admit requests the pool could never hold, and the run-ahead loop then span on a burst that could not succeed).
        st0 = self.kv_stats()
        pool_pages = st0["total_pages"]
        total_pages = st0["free_pages"]
        need_pages = [(sp.max_length - 1 + NTTS_PAGE_TOKENS - 1) // NTTS_PAGE_TOKENS for sp in sampling]
        for i, n in enumerate(need_pages):
            if n > total_pages:
                raise NeuTTSHipError(-3, f"prompt {i}: max_length {sampling[i].max_length} needs {n} KV pages, the pool has {total_pages} free of {pool_pages}")
        committed: Dict[int, int] = {}                      # slot -> pages reserved for it
        results: List[Optional[List[int]]] = [None] * len(prompts)
        logps: List[Optional[np.ndarray]] = [None] * len(prompts)
        owner: Dict[int, int] = {}
        anchors: List[tuple] = []       # (slot, prompt as int32 array) of live slots that later prompts are compared with
        arrs = [np.asarray(p, dtype=np.int32) for p in prompts] if share_prefix else None
        # run-ahead bookkeeping: snapshots are numbered in stream order; a slot's entry in snapshot q describes the request that
        # owns it now only if the slot was (re)filled before snapshot q was enqueued
        snap_seq = 0                    # number of the next snapshot to be enqueued
        valid_from: Dict[int, int] = {}  # slot -> first snapshot number that describes its current request
        steps_left: Dict[int, int] = {}  # slot -> decode steps its request can still take before max_length stops it (run-ahead: upper bound)
        open_snap: Optional[int] = None  # number of the snapshot opened by poll_begin and not read yet

        def find_donor(i):
            best = None
            for slot, arr in anchors:
                m = min(len(arr), len(arrs[i]) - 1)
                if m < NTTS_PAGE_TOKENS:
                    continue
                neq = np.flatnonzero(arr[:m] != arrs[i][:m])
                lcp = int(neq[0]) if len(neq) else m
                if lcp >= NTTS_PAGE_TOKENS and (best is None or lcp > best[1]):
                    best = (slot, lcp)
            return best

        nxt = 0

        # Parking (cfg["park_slots"] > 0): a prompt pass may also fill PARKING rows -- the requests wait there, prefilled, and move into a decode slot
        # the moment one is released.  Admission then counts the free parking rows as well: the waves of `min_admit` prompts keep their
        # efficient size while no decode row idles waiting for the next wave (slot occupancy 0.92 -> ~0.99: bench.py --mode continuous).
        from collections import deque
        parked: "deque[int]" = deque()   # parking rows holding a prefilled request, oldest first

        def n_free():
            return len(self._free) + len(self._free_park)

        def may_admit():
            if not owner:
                return True
            want = min(min_admit, len(prompts) - nxt)
            return admit_gate(n_free(), want) if admit_gate is not None else n_free() >= want

        def activate_parked():
            """parked requests into the decode slots that are free right now; their bookkeeping moves along"""
            nonlocal anchors
            rows, slots_ = [], []
            while parked and self._free:
                rows.append(parked.popleft())
                slots_.append(self.acquire_slot())
            if not rows:
                return
            self.activate(rows, slots_)
            for r, s in zip(rows, slots_):
                owner[s] = owner.pop(r)
                committed[s] = committed.pop(r)
                steps_left[s] = steps_left.pop(r)
                valid_from.pop(r, None)
                valid_from[s] = snap_seq                  # the snapshots enqueued from here on describe it in its decode slot
                anchors = [(s if a[0] == r else a[0], a[1]) for a in anchors]

        try:
            while nxt < len(prompts) or owner:
                # admit as many waiting prompts as slots / prefill workspace allow
                while nxt < len(prompts) and n_free() and may_admit():
                    batch, used, donors = [], 0, []
                    while nxt < len(prompts) and n_free():
                        d = find_donor(nxt) if share_prefix else None
                        cost = len(prompts[nxt]) - (d[1] // NTTS_PAGE_TOKENS * NTTS_PAGE_TOKENS if d else 0)
                        if used + cost > budget or sum(committed.values()) + need_pages[nxt] > total_pages:
                            break
                        s = self.acquire_slot() if self._free else self.acquire_park()    # decode slots first, then parking rows
                        if s >= self.max_batch:
                            parked.append(s)
                        committed[s] = need_pages[nxt]
                        batch.append((nxt, s))
                        donors.append(d)
                        used += cost
                        owner[s] = nxt
                        valid_from[s] = snap_seq
                        steps_left[s] = sampling[nxt].max_length - len(prompts[nxt]) - 1
                        if share_prefix and d is None and len(anchors) < 16:
                            anchors.append((s, arrs[nxt]))      # a new beginning: later prompts may share it
                        nxt += 1
                    if not batch:
                        break
                    try:
                        self.prefill([prompts[i] for i, _ in batch], [s for _, s in batch], [sampling[i] for i, _ in batch],
                                     donors if share_prefix else None)
                    except NeuTTSHipError as ex:
                        running = [s for s in owner if s not in [b[1] for b in batch]]
                        if ex.code != -3 or not running:
                            raise
                        # KV page pool exhausted while other requests still run: hand this batch back, let the running
                        # ones finish and free their pages, then try again
                        for i, s in reversed(batch):
                            owner.pop(s)
                            steps_left.pop(s, None)
                            committed.pop(s, None)
                            anchors = [a for a in anchors if a[0] != s]
                            if s >= self.max_batch:
                                parked.remove(s)
                                self._free_park.append(s)
                            else:
                                self._free.append(s)
                        nxt = batch[0][0]
                        break
                    if on_admit is not None:
                        on_admit(len(batch))
                if not owner:
                    raise NeuTTSHipError(-4, "no decode slot is free (held by an unfinished stream?)")
                activate_parked()                                 # (decode slots freed in the previous iteration)
                if run_ahead:
                    # keep the GPU fed: this burst goes in BEFORE the host looks at the previous burst's outcome.  Stream order per
                    # iteration j: [prompt pass j] [burst j] [exports / releases j] [snapshot j]; the host waits for snapshot j - 1
                    # only, with burst j queued behind it.  No burst when every owner has certainly stopped already (each has been
                    # given the decode steps its max_length allows: the snapshots in flight will show them finished).
                    burst_failed = None
                    if any(steps_left.get(s, 1) > 0 for s in owner if s < self.max_batch):
                        try:
                            self.decode(steps_per_poll)
                            for s in owner:
                                if s < self.max_batch:            # (parked requests take no decode steps)
                                    steps_left[s] = steps_left.get(s, 0) - steps_per_poll
                        except NeuTTSHipError as ex:
                            # Running one burst ahead, rows that have finished on the device still count as running on the host and
                            # ntts_backbone_decode reserves KV pages for them (up to one page per slot): with a tightly sized pool that
                            # can fail where the blocking scheduler succeeds.  Nothing was enqueued: drain the snapshot in flight,
                            # release what has finished, and try again on the next iteration.
                            if ex.code != -3:
                                raise
                            burst_failed = ex
                    if open_snap is None:
                        st = nn = None
                        if burst_failed is not None:
                            st, nn = self.poll()                      # blocking: everything enqueued so far
                            q = snap_seq
                            if not any(st[s] == 2 for s in owner if s < self.max_batch):
                                raise burst_failed                    # nothing to drain: the pool really is too small
                    else:
                        st, nn = self.poll_end()
                        q, open_snap = open_snap, None
                        if burst_failed is not None and not any(valid_from.get(s, 0) <= q and st[s] == 2 for s in owner if s < self.max_batch):
                            # the burst could not reserve its pages and the snapshot in flight frees nothing: look at everything
                            # enqueued so far; if no owner has finished there either, no later iteration can cure it (ADVICE r4:
                            # this used to spin on poll_end / poll_begin forever, and an EngineGang with it)
                            st, nn = self.poll()
                            q = snap_seq
                            if not any(st[s] == 2 for s in owner if s < self.max_batch):
                                raise burst_failed
                else:
                    st, nn = self.poll()
                    q = snap_seq                                  # a blocking poll describes everything enqueued so far
                if st is not None:
                    for s in [s for s in list(owner) if s < self.max_batch and valid_from.get(s, 0) <= q and st[s] == 2]:
                        i = owner.pop(s)
                        if return_logprobs:
                            logps[i] = self.read_finished_logprobs(s) if run_ahead else self.read_logprobs(s)
                        if on_finished is not None:
                            on_finished(i, s, int(nn[s]))
                            results[i] = []
                        else:
                            results[i] = self.read_finished(s) if run_ahead else self.read(s)[0]
                        committed.pop(s, None)
                        self.release(s)                          # shared pages live on until their last user is released
                        valid_from.pop(s, None)
                        steps_left.pop(s, None)
                        anchors = [a for a in anchors if a[0] != s]
                if run_ahead:
                    self.poll_begin()
                    open_snap = snap_seq
                    snap_seq += 1
                elif owner and (parked or any(st[s] == 1 for s in owner if s < self.max_batch)):
                    activate_parked()
                    self.decode(steps_per_poll)
                yield None
        finally:
            # an exception (KV pool exhausted, a failed launch, ...) must not leave admitted slots RUNNING with their
            # pages held: the next call would find them busy
            if open_snap is not None:
                try:
                    self.poll_end()
                except NeuTTSHipError:
                    pass
            if owner:
                try:
                    self.sync()
                except NeuTTSHipError:
                    pass
                for s in list(owner):
                    try:
                        self.release(s)
                    except NeuTTSHipError:
                        pass
        ids = [r if r is not None else [] for r in results]
        if return_logprobs:
            return ids, [lp if lp is not None else np.zeros(0, dtype=np.float32) for lp in logps]
        return ids


class EngineGang:
    """Several BackboneEngines on ONE set of weights, run side by side on one GPU.  A decode step is a chain of 171 dependent
    launches of 5-20 us each, latency-bound at a quarter of the HBM peak; several such chains on streams of their own fill each
    other's launch gaps and first round trips (MI355X, 256 rows at context 625: 1.57 ms per step alone, 1.11 / 1.02 / 0.96 ms per
    256-row step with two / three / four chains).  The gang creates n - 1 twins of `engine` that read its arena
    (ntts_backbone_share_arena: KV pool, slots, workspaces and step graph per engine, the weights once), gives every engine a lane
    stream of its own for all of its work -- the HIP runtime multiplexes streams onto FOUR hardware queues (more make it slower), and
    two chains in one queue run one after the other, so n <= 4 and the lanes are created back to back -- and alternates between the
    engines' schedulers from the calling thread.  Each request's arithmetic is that of a single engine (same kernels, same
    slots per engine): ids are identical to BackboneEngine.generate's."""

    MAX_ENGINES = 4        # hardware queues the HIP runtime multiplexes streams onto: a fifth chain shares a queue and the gang gets SLOWER

    def __init__(self, engine: "BackboneEngine", n: int = 4, lanes: bool = True):
        if not 1 <= n <= self.MAX_ENGINES:
            raise ValueError(f"an engine gang has 1..{self.MAX_ENGINES} engines (one hardware queue each), not {n}")
        self.lib, self._device = engine.lib, engine._device
        self._streams: List[int] = []
        self.engines: List[BackboneEngine] = [engine]
        try:
            for _ in range(n - 1):
                self.engines.append(engine.twin())
            if lanes and n > 1:
                for _ in range(n):                       # created back to back: up to four streams land in distinct hardware queues
                    st = C.c_void_p()
                    rc = self.lib.ntts_stream_create(self._device, C.byref(st))
                    if rc != 0:
                        raise NeuTTSHipError(rc, "ntts_stream_create failed")
                    self._streams.append(st.value)
                for e, st in zip(self.engines, self._streams):
                    e.set_stream(st)
            # (the decode step's tile family depends on how many chains share the chip: since ABI 9 every engine counts them itself at each
            #  decode call -- ntts_backbone_set_gang only pins the count for tests and sweeps -- so an engine of the gang that decodes alone
            #  for a while, e.g. NeuTTS.infer on engine 0, runs the single-chain shape meanwhile)
        except Exception:
            self.close()                                 # twins and lanes made so far must not leak
            raise

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def lane(self, k: int) -> Optional[int]:
        """Engine k's lane stream (lend it to that engine's codec engine too: CodecEngine.set_stream), None without lanes."""
        return self._streams[k] if self._streams else None

    @property
    def max_batch(self) -> int:
        return sum(e.max_batch for e in self.engines)

    def warm_up(self, decode_steps: int = 2):
        for e in self.engines:
            e.warm_up(decode_steps)

    def generate(self, prompts: Sequence[Sequence[int]], sampling, on_finished=None, steps_per_poll: int = 1, admit: str = "wave",
                 on_admit=None, return_logprobs: bool = False, **kw) -> List[List[int]]:
        """BackboneEngine.generate over the gang: request i goes to engine i % n (prompts of one speaker that follow each other n apart
        still share their prefix pages inside an engine), the engines' schedulers advance in turn.  Bursts of `steps_per_poll` = 1 step
        by default: the engines' bursts are enqueued in turn, and the shorter the turn the closer their chains run side by side (8192
        ragged requests, round 4: 144.5 k codec-tokens/s at 1-2 steps, 132.0 k at 4, 106.7 k at 8, profiles/r04s_sweep_continuous_gang_sched.txt;
        round 5 with admission waves: 149.8 k at 1, 146.3-147.0 k at 2).  on_finished(request index, slot, n_new, engine) -- the engine is
        passed along for the device-side hand-off.  Returns the new ids in request order; with return_logprobs=True (every engine's set_logprobs
        on) the pair (ids, logprobs), as BackboneEngine.generate does.
        admit: how the engines' prompt passes are placed against each other once `min_admit` > 1 (a pass holds its engine's lane for
        ~ 0.8 us per prompt token while the other chains go on).  "wave[:F[:W]]" (default) -- when one engine admits `min_admit`
        prompts, the others admit within W rounds (default 1) with min_admit / F (default a third) of their slots free: all prompt
        passes at once, then four decode chains side by side again, the static schedule's pattern -- 149.8 k against 145.6 k for
        "independent" (each engine admits when `min_admit` of ITS slots are free; steady state 156.3 k against 149.7 k), flat over
        min_admit 20-28, F 2-3, W 1-2; "spaced:R" -- not within R rounds of ANY engine's last pass (at most one engine out of the
        decode gang at a time): 142.0 k at R = 3, 121.5 k at 6 (profiles/r05m_sweep_continuous_admission_*.txt).  Scheduling only:
        ids cannot differ.  on_admit(engine, n_prompts): called after each prompt pass of an engine is enqueued (the moment to put
        other lane-holding work of that engine -- a codec pass over what it has finished -- next to the wave)."""
        n = len(self.engines)
        sched = {"round": 0, "last": -(1 << 30)}
        space, follow, window = 0, 3, 1
        try:
            kind, *num = admit.split(":")
            num = [int(x) for x in num]
            if kind == "spaced" and len(num) == 1 and num[0] > 0:
                space = num[0]
            elif kind == "wave" and len(num) <= 2 and all(x > 0 for x in num):
                follow, window = (num + [3, 1][len(num):])
            elif kind != "independent" or num:
                raise ValueError
        except ValueError:
            raise ValueError(f"admit = {admit!r}: 'independent', 'spaced:<rounds>' or 'wave[:<follower divisor>[:<rounds>]]'") from None

        def gate(n_free, want):
            if space:
                return n_free >= want and sched["round"] - sched["last"] >= space
            return n_free >= want or (sched["round"] - sched["last"] <= window and n_free >= max(1, want // follow))

        def admitted(n_prompts):
            if space or n_prompts >= kw.get("min_admit", 1):     # (a follower's small pass does not re-arm the wave)
                sched["last"] = sched["round"]
        if admit != "independent":
            kw = dict(kw, admit_gate=gate)
        if isinstance(sampling, Sampling):
            sampling = [sampling] * len(prompts)
        parts = [list(range(k, len(prompts), n)) for k in range(n)]
        its = []
        for e, idx in zip(self.engines, parts):
            if not idx:
                continue
            hook = None
            if on_finished is not None:
                hook = (lambda i, slot, n_new, _e=e, _idx=idx: on_finished(_idx[i], slot, n_new, _e))
            note = None
            if admit != "independent" or on_admit is not None:
                def note(n_prompts, _e=e):
                    if admit != "independent":
                        admitted(n_prompts)
                    if on_admit is not None:
                        on_admit(_e, n_prompts)
            its.append((idx, e.generate_iter([prompts[i] for i in idx], [sampling[i] for i in idx], steps_per_poll=steps_per_poll, on_finished=hook,
                                             on_admit=note, return_logprobs=return_logprobs, **kw)))
        results: List[List[int]] = [[] for _ in prompts]
        logps: List[np.ndarray] = [np.zeros(0, dtype=np.float32) for _ in prompts]
        try:
            while its:
                sched["round"] += 1
                for item in list(its):
                    idx, it = item
                    try:
                        next(it)
                    except StopIteration as done:
                        ids, lps = done.value if return_logprobs else (done.value, None)
                        for k, i in enumerate(idx):
                            results[i] = ids[k]
                            if lps is not None:
                                logps[i] = lps[k]
                        its.remove(item)
        finally:
            for _, it in its:
                it.close()                                # an exception in one engine: the others release their slots (generate_iter's finally)
        return (results, logps) if return_logprobs else results

    def sync(self):
        for e in self.engines:
            e.sync()

    def close(self):
        """Twins destroyed, engine 0 back on its own stream and its single-chain tiles, lanes destroyed.  Idempotent."""
        engines, self.engines = getattr(self, "engines", []), getattr(self, "engines", [])[:1]
        for e in reversed(engines[1:]):
            e.close()
        if engines and getattr(engines[0], "h", None):
            if self._streams:
                engines[0].set_stream(None)
            engines[0].set_gang(0)
        for st in self._streams:
            self.lib.ntts_stream_destroy(self._device, C.c_void_p(st))
        self._streams = []


class CodecEngine:
    """NeuCodec decoder on one GPU: codes -> 24 kHz waveform (replaces codec.decode_code, ref:neutts/neutts.py:288-291)."""

    def __init__(self, cfg: dict, device: int = 0, lib_path: Optional[str] = None):
        self.lib = load_library(lib_path)
        lv = list(cfg.get("levels", [4] * 8))
        c = CodecConfigC(cfg.get("hidden_size", 1024), cfg.get("intermediate_size", 4096), cfg.get("num_layers", 12),
                         cfg.get("num_heads", 16), cfg.get("head_dim", 64), cfg.get("quantization_dim", 2048), len(lv),
                         (C.c_int32 * 8)(*(lv + [1] * (8 - len(lv)))), cfg.get("hop_length", 480), cfg.get("rms_eps", 1e-6),
                         cfg.get("max_frames", 2048), cfg.get("max_rows", 4096),
                         {"fp16": 0, "high": 1, "bf16": 2, 0: 0, 1: 1, 2: 2}[cfg.get("precision", "fp16")])
        h = C.c_void_p()
        rc = self.lib.ntts_codec_create(C.byref(c), device, C.byref(h))
        if rc != 0:
            raise NeuTTSHipError(rc, (self.lib.ntts_codec_last_error(None) or b"").decode())
        self.h = h
        self.hop_length = c.hop_length
        self.max_frames, self.max_rows = c.max_frames, c.max_rows
        self.device = device

    def _chk(self, rc: int):
        if rc != 0:
            raise NeuTTSHipError(rc, (self.lib.ntts_codec_last_error(self.h) or b"").decode())

    def close(self):
        if getattr(self, "_pin_ptr", None):
            self.lib.ntts_host_free(self._pin_ptr)
            self._pin_ptr, self._pin_cap = None, 0
        if getattr(self, "h", None):
            self.lib.ntts_codec_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load_state_dict(self, sd: Dict[str, object]):
        for k, v in sd.items():
            ptr, code, shape, is_dev, keep = _tensor_ptr(v)
            shp = (C.c_int64 * len(shape))(*shape)
            self._chk(self.lib.ntts_codec_load_tensor(self.h, k.encode(), C.c_void_p(ptr), code, shp, len(shape), is_dev))
            del keep
        self._chk(self.lib.ntts_codec_finalize(self.h))

    def _pinned(self, n: int, dtype=np.float32) -> np.ndarray:
        """Engine-owned page-locked staging buffer (sized in bytes, grown on demand), viewed as a numpy array of `n` elements of `dtype`."""
        nbytes = max(1, n * np.dtype(dtype).itemsize)
        if getattr(self, "_pin_cap", 0) < nbytes:
            if getattr(self, "_pin_ptr", None):
                self.lib.ntts_host_free(self._pin_ptr)
                self._pin_ptr, self._pin_cap = None, 0
            ptr = C.c_void_p()
            if self.lib.ntts_host_alloc(nbytes, C.byref(ptr)) != 0:
                raise MemoryError("pinned host allocation failed")
            self._pin_ptr, self._pin_cap = ptr, nbytes
        return np.frombuffer((C.c_char * nbytes).from_address(self._pin_ptr.value), dtype=dtype, count=n)

    def _row_len(self, lens: np.ndarray, fc, pm: Optional[np.ndarray]) -> int:
        """Samples of the longest utterance of a decode call in the format `fc`, behind the stretch at the speeds pm (None: all 1000)."""
        if pm is None:
            return wav_out_len(self.hop_length * int(lens.max()), fc.sample_rate)
        return wav_out_len(max(wav_stretch_len(self.hop_length * int(t), int(s)) for t, s in zip(lens, pm)), fc.sample_rate)

    def _decode_entry(self, n: int, codes, lens: np.ndarray, fmt, pm: Optional[np.ndarray], loud, dst: int, stride: int, dev=None):
        """The one C call of `decode` (codes: the packed int32 array) and of `decode_device` (codes: a device pointer; dev = (codes_stride,
        destination on the device, producer stream)) -> samples per utterance.  The native format at speed 1 without a loudness is
        ntts_codec_decode / ntts_codec_decode_dev: the calls and the bits of an engine without the stages.  Everything else is
        ntts_codec_decode_loud / ntts_codec_decode_dev_loud with null for the stages that are off (the C side makes the very same calls for them).
        A new stage of the output path gets its argument here."""
        fc, _, native = fmt
        i32p = C.POINTER(C.c_int32)
        src = C.c_void_p(codes) if dev else codes.ctypes.data_as(i32p)
        if native and pm is None and loud is None:
            if dev:
                self._chk(self.lib.ntts_codec_decode_dev(self.h, n, src, dev[0], lens.ctypes.data_as(i32p), C.c_void_p(dst), stride, dev[1],
                                                         C.c_void_p(dev[2] or None)))
            else:
                self._chk(self.lib.ntts_codec_decode(self.h, n, src, lens.ctypes.data_as(i32p), C.cast(C.c_void_p(dst), C.POINTER(C.c_float)), stride))
            return self.hop_length * lens.astype(np.int64)
        out_lens = np.zeros(n, dtype=np.int32)
        sp = None if pm is None else pm.ctypes.data_as(i32p)
        if dev:
            self._chk(self.lib.ntts_codec_decode_dev_loud(self.h, n, src, dev[0], lens.ctypes.data_as(i32p), sp, loud, C.c_void_p(dst), stride, dev[1],
                                                          C.c_void_p(dev[2] or None), C.byref(fc), out_lens.ctypes.data_as(i32p)))
        else:
            self._chk(self.lib.ntts_codec_decode_loud(self.h, n, src, lens.ctypes.data_as(i32p), sp, loud, C.byref(fc), C.c_void_p(dst), stride,
                                                      out_lens.ctypes.data_as(i32p)))
        return out_lens

    def _decode_call(self, n: int, flat: np.ndarray, lens: np.ndarray, fmt, reuse_output: bool, pm: Optional[np.ndarray] = None, loud=None):
        """One decode call on packed host codes -> ([n, stride] array of the format's dtype, samples per utterance).  pm: speeds per mille
        (int32 [n]) or None; loud: an ntts_wav_loudness array [n] or None."""
        if pm is not None:
            pm = np.ascontiguousarray(pm, dtype=np.int32)
        stride = self._row_len(lens, fmt[0], pm)
        wav = (self._pinned(n * stride, fmt[1]) if reuse_output else np.empty(n * stride, dtype=fmt[1])).reshape(n, stride)
        return wav, self._decode_entry(n, flat, lens, fmt, pm, loud, wav.ctypes.data, stride)

    def decode(self, codes: Sequence[Sequence[int]], reuse_output: bool = False, sample_rate=None, encoding="f32",
               filter_width=None, speed=None, loudness=None, loudness_peak=LOUDNESS_PEAK_DEFAULT,
               loudness_max_gain=LOUDNESS_MAX_GAIN_DEFAULT) -> List[np.ndarray]:
        """codes: one int sequence per utterance -> list of waveforms: float32 at 24 kHz, hop_length * len samples each, by default;
        sample_rate (one of WAV_RATES) / encoding ("f32", "pcm16" -> int16, "mulaw" -> uint8) / filter_width (the resampler's
        lowpass_filter_width, 1..64, default 6) put the device output stage behind the pass: ceil(hop_length * len * rate / 24000) samples.
        speed (0.5 .. 2.0, one value or one per utterance; None = 1.0) puts the time stretch between the pass and the output stage: the pitch stays,
        the utterance takes ceil(hop_length * len / speed) samples at 24 kHz.
        loudness (a target in LUFS, -70 .. 0, one value or one per utterance; None or a None entry = off) puts the BS.1770 loudness normalisation
        between the stretch and the output stage: one gain per utterance, held by loudness_max_gain (dB) and by the sample-peak ceiling
        loudness_peak (dBFS) (ntts_codec_decode_loud, the entry point of every call with a stage on).
        reuse_output=True returns views into an engine-owned pinned buffer (fast D2H, no copy): they are only valid
        until the next decode() call on this engine."""
        fmt = wav_format(sample_rate, encoding, filter_width)
        pm = speed_permille(speed, len(codes))
        loud = loudness_params(loudness, loudness_peak, loudness_max_gain, len(codes))
        out: List[Optional[np.ndarray]] = [None] * len(codes)
        order = sorted(range(len(codes)), key=lambda i: -len(codes[i]))   # batch similar lengths together
        i = 0
        while i < len(order):
            tmax = len(codes[order[i]])
            nb = max(1, min(len(order) - i, self.max_rows // (tmax + 6)))
            grp = order[i:i + nb]
            lens = np.array([len(codes[j]) for j in grp], dtype=np.int32)
            flat = np.ascontiguousarray(np.concatenate([np.asarray(codes[j], dtype=np.int32) for j in grp]))
            # (pinned fast path when a single call covers the batch)
            wav, out_lens = self._decode_call(len(grp), flat, lens, fmt, reuse_output and i == 0 and nb == len(order),
                                              None if pm is None else pm[grp], None if loud is None else _loudness_rows(loud, grp))
            for r, j in enumerate(grp):
                out[j] = wav[r, : int(out_lens[r])]     # view into this call's buffer: no second copy
            i += nb
        return out  # type: ignore[return-value]

    def decode_array(self, codes: np.ndarray, lens: Optional[np.ndarray] = None, reuse_output: bool = False, sample_rate=None,
                     encoding="f32", filter_width=None, speed=None) -> np.ndarray:
        """Batch fast path: codes [n, T] int (row i valid up to lens[i]; all T when lens is None) -> waveforms
        [n, hop_length * T] float32 in ONE engine call (n * (T + 6) must fit max_rows).  reuse_output=True returns a
        view of the engine's pinned staging buffer, valid until the next decode on this engine.  With an output format (as `decode`):
        [n, wav_out_len(hop_length * T, sample_rate)] of the encoding's dtype, row i valid up to wav_out_len(hop_length * lens[i], sample_rate);
        with speed (as `decode`) the row length is the longest stretched utterance's."""
        fmt = wav_format(sample_rate, encoding, filter_width)
        codes = np.asarray(codes)
        n, T = codes.shape
        pm = speed_permille(speed, n)
        if lens is None:
            lens = np.full(n, T, dtype=np.int32)
            flat = np.ascontiguousarray(codes, dtype=np.int32).reshape(-1)
        else:
            lens = np.ascontiguousarray(lens, dtype=np.int32)
            flat = np.ascontiguousarray(np.concatenate([codes[i, : lens[i]] for i in range(n)]), dtype=np.int32)
        return self._decode_call(n, flat, lens, fmt, reuse_output, pm)[0]

    def stretch_array(self, wav: np.ndarray, n_samples, speed, sample_rate=None, encoding="f32", filter_width=None, out_stride: Optional[int] = None,
                      pos_stride: Optional[int] = None):
        """The time stretch alone, and the output stage behind it (ntts_codec_stretch): wav [n, in_stride] float32 at 24 kHz, row i valid up to
        n_samples[i], speed one value or one per row -> ([n, out_stride] array of the encoding's dtype, samples per row, positions [n, pos_stride]
        int32, frames per row): row i's positions p_0 .. p_{K_i - 1} are the input offsets its output frames of 360 samples were taken from."""
        fc, dtype, wav, n_samples = self._array_args(wav, n_samples, sample_rate, encoding, filter_width)
        n, in_stride = wav.shape
        pm = speed_permille(speed, n)
        if pm is None:
            pm = np.full(n, 1000, dtype=np.int32)
        s_len = [wav_stretch_len(max(0, int(v)), int(s)) for v, s in zip(n_samples, pm)]
        buf, out_stride, out_lens = self._out_rows(n, out_stride, max(s_len) if n else 0, fc, dtype)
        if pos_stride is None:
            pos_stride = -(-(max(s_len) if n else 0) // STRETCH_HOP)
        pos_stride = int(pos_stride)
        pos = np.full(max(1, n * max(0, pos_stride)), -1, dtype=np.int32)
        i32p = C.POINTER(C.c_int32)
        self._chk(self.lib.ntts_codec_stretch(self.h, n, wav.ctypes.data_as(C.POINTER(C.c_float)), in_stride, n_samples.ctypes.data_as(i32p),
                                              pm.ctypes.data_as(i32p), C.byref(fc), C.c_void_p(buf.ctypes.data), out_stride,
                                              out_lens.ctypes.data_as(i32p), pos.ctypes.data_as(i32p), pos_stride))
        frames = np.array([-(-v // STRETCH_HOP) for v in s_len], dtype=np.int32)
        return buf[: n * out_stride].reshape(n, out_stride), out_lens, pos[: n * pos_stride].reshape(n, pos_stride), frames

    def stretch(self, wavs: Sequence[np.ndarray], speed, sample_rate=None, encoding="f32", filter_width=None) -> List[np.ndarray]:
        """24 kHz float waveforms (one 1-D array each; e.g. what a watermarker handed back) -> the same `speed` times faster, pitch kept, in the
        output format: what `decode` with these arguments would have produced from them."""
        buf, n_samples = self._rows_of(wavs)
        if not len(buf):
            return []
        out, out_lens, _, _ = self.stretch_array(buf, n_samples, speed, sample_rate, encoding, filter_width)
        return [out[r, : int(out_lens[r])] for r in range(len(buf))]

    def last_stretch_timing(self):
        """GPU milliseconds (search kernel, render kernel) of the most recent time stretch on this engine."""
        a, b = C.c_float(), C.c_float()
        self._chk(self.lib.ntts_codec_last_stretch_timing(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    @staticmethod
    def _rows_of(wavs):
        """Waveforms (one 1-D array each) -> ([n, longest] float32 with zeros behind each row, samples per row): what `stretch`, `convert`,
        `normalize` and `measure_loudness` hand to the engine."""
        wavs = [np.asarray(w, dtype=np.float32).reshape(-1) for w in wavs]
        n_samples = np.array([len(w) for w in wavs], dtype=np.int32)
        buf = np.zeros((len(wavs), max(1, int(n_samples.max(initial=0)))), dtype=np.float32)
        for r, w in enumerate(wavs):
            buf[r, : len(w)] = w
        return buf, n_samples

    @staticmethod
    def _array_args(wav, n_samples, sample_rate, encoding, filter_width):
        """The checked arguments of `stretch_array` and `convert_array` -> (WavFormatC, dtype, wav [n, in_stride] float32, n_samples int32 [n])."""
        fc, dtype, _ = wav_format(sample_rate, encoding, filter_width)
        wav = np.ascontiguousarray(wav, dtype=np.float32)
        n, _ = wav.shape
        n_samples = np.ascontiguousarray(n_samples, dtype=np.int32)
        if len(n_samples) != n:
            raise ValueError(f"n_samples: {len(n_samples)} values for {n} waveforms")
        return fc, dtype, wav, n_samples

    @staticmethod
    def _out_rows(n: int, out_stride: Optional[int], longest: int, fc, dtype):
        """Their destination -> (zeroed flat buffer of n rows, out_stride, out_lens); out_stride None: the `longest` row's samples in the format."""
        out_stride = int(wav_out_len(longest, fc.sample_rate) if out_stride is None else out_stride)
        buf = np.zeros(max(1, n * max(0, out_stride)), dtype=dtype)       # (never a null pointer, even for n rows of no samples)
        return buf, out_stride, np.zeros(n, dtype=np.int32)

    def normalize(self, wavs: Sequence[np.ndarray], loudness, loudness_peak=LOUDNESS_PEAK_DEFAULT, loudness_max_gain=LOUDNESS_MAX_GAIN_DEFAULT,
                  sample_rate=None, encoding="f32", filter_width=None, return_measured: bool = False):
        """24 kHz float waveforms (one 1-D array each; e.g. what a watermarker handed back) -> the same at the loudness `decode` with these arguments
        would have given them, in the output format (ntts_codec_normalize).  return_measured=True: (waveforms, float64 [n, 3]) with row i =
        (integrated loudness in LUFS, NaN where the row is unmeasurable; sample peak; the gain applied)."""
        buf, n_samples = self._rows_of(wavs)
        n = len(buf)
        fc, dtype, _ = wav_format(sample_rate, encoding, filter_width)
        loud = loudness_params(loudness, loudness_peak, loudness_max_gain, n)
        if not n:
            return ([], np.zeros((0, 3))) if return_measured else []
        if loud is None:
            loud = (WavLoudnessC * n)()
        out_stride = wav_out_len(int(n_samples.max()), fc.sample_rate)
        out = np.zeros((n, max(1, out_stride)), dtype=dtype)
        out_lens = np.zeros(n, dtype=np.int32)
        measured = np.zeros((n, 3), dtype=np.float64)
        i32p = C.POINTER(C.c_int32)
        self._chk(self.lib.ntts_codec_normalize(self.h, n, buf.ctypes.data_as(C.POINTER(C.c_float)), buf.shape[1], n_samples.ctypes.data_as(i32p),
                                                loud, C.byref(fc), C.c_void_p(out.ctypes.data), out.shape[1], out_lens.ctypes.data_as(i32p),
                                                measured.ctypes.data_as(C.POINTER(C.c_double)) if return_measured else None))
        res = [out[r, : int(out_lens[r])] for r in range(n)]
        return (res, measured) if return_measured else res

    def measure_loudness(self, wavs: Sequence[np.ndarray]) -> np.ndarray:
        """24 kHz float waveforms -> float64 [n, 3]: row i = (BS.1770-4 integrated loudness in LUFS, NaN where unmeasurable; sample peak max|x|; 1.0).
        Nothing is scaled (ntts_codec_measure_loudness)."""
        buf, n_samples = self._rows_of(wavs)
        measured = np.zeros((len(buf), 3), dtype=np.float64)
        if not len(buf):
            return measured
        self._chk(self.lib.ntts_codec_measure_loudness(self.h, len(buf), buf.ctypes.data_as(C.POINTER(C.c_float)), buf.shape[1],
                                                       n_samples.ctypes.data_as(C.POINTER(C.c_int32)), measured.ctypes.data_as(C.POINTER(C.c_double))))
        return measured

    def last_loudness_timing(self):
        """GPU milliseconds (measure kernel, apply kernel) of the most recent loudness stage on this engine."""
        a, b = C.c_float(), C.c_float()
        self._chk(self.lib.ntts_codec_last_loudness_timing(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def convert_array(self, wav: np.ndarray, n_samples, sample_rate=None, encoding="f32", filter_width=None, out_stride: Optional[int] = None):
        """The output stage alone (ntts_codec_convert): wav [n, in_stride] float32 at 24 kHz, row i valid up to n_samples[i] (what follows is
        never read as signal) -> ([n, out_stride] array of the encoding's dtype, samples per row)."""
        fc, dtype, wav, n_samples = self._array_args(wav, n_samples, sample_rate, encoding, filter_width)
        n, in_stride = wav.shape
        buf, out_stride, out_lens = self._out_rows(n, out_stride, max(0, int(n_samples.max(initial=0))), fc, dtype)
        i32p = C.POINTER(C.c_int32)
        self._chk(self.lib.ntts_codec_convert(self.h, n, wav.ctypes.data_as(C.POINTER(C.c_float)), in_stride, n_samples.ctypes.data_as(i32p),
                                              C.byref(fc), C.c_void_p(buf.ctypes.data), out_stride, out_lens.ctypes.data_as(i32p)))
        out = buf[: n * out_stride].reshape(n, out_stride)
        return out, out_lens

    def convert(self, wavs: Sequence[np.ndarray], sample_rate=None, encoding="f32", filter_width=None) -> List[np.ndarray]:
        """24 kHz float waveforms (one 1-D array each; e.g. what a watermarker handed back) -> the same in another output format, as `decode`
        with these arguments would have produced from them."""
        buf, n_samples = self._rows_of(wavs)
        if not len(buf):
            return []
        out, out_lens = self.convert_array(buf, n_samples, sample_rate, encoding, filter_width)
        return [out[r, : int(out_lens[r])] for r in range(len(buf))]

    def stream_stretcher(self, n: int = 1, speed=1.0, sample_rate=None, encoding="f32", filter_width=None, max_chunk_samples: int = 16384) -> "SpeedStream":
        """The time stretch, and the output stage behind it, for `n` signals that arrive in chunks (ntts_speed_stream_*): the streaming twin of
        `stretch`.  speed: one value or one per stream, the default of `push`."""
        return SpeedStream(self, n, speed, sample_rate, encoding, filter_width, max_chunk_samples)

    def stream_converter(self, n: int = 1, sample_rate=None, encoding="f32", filter_width=None, max_chunk_samples: int = 16384) -> "WavStream":
        """The output stage for `n` signals that arrive in chunks (ntts_wav_stream_*): the streaming twin of `convert`."""
        return WavStream(self, n, sample_rate, encoding, filter_width, max_chunk_samples)

    def set_debug(self, keep_stages: bool):
        self._chk(self.lib.ntts_codec_set_debug(self.h, int(keep_stages)))

    STAGES = ["embed", "prior", "layers", "post"]            # the tap names of oracle/codec_ref.py decode_code(taps=...)

    def read_stage(self, stage: int, utt: int = 0) -> np.ndarray:
        """fp32 residual stream [frames, hidden] of utterance `utt` after stage `stage` of the most recent decode call (set_debug(True) first)."""
        buf = np.empty(self.max_frames * 4096, dtype=np.float32)
        r, c_ = C.c_int32(), C.c_int32()
        self._chk(self.lib.ntts_codec_read_stage(self.h, stage, utt, buf.ctypes.data_as(C.POINTER(C.c_float)), buf.size, C.byref(r), C.byref(c_)))
        return buf[: r.value * c_.value].reshape(r.value, c_.value).copy()

    def set_cu_mask(self, mask_words: Optional[Sequence[int]]):
        """Restrict the codec engine's stream to the CUs of `mask_words` (None / empty = all); ntts_codec_set_cu_mask."""
        words = list(mask_words or [])
        arr = (C.c_uint32 * max(1, len(words)))(*words)
        self._chk(self.lib.ntts_codec_set_cu_mask(self.h, arr, len(words)))

    def decode_device(self, codes_dev_ptr: int, codes_stride: int, lens: np.ndarray, producer_stream: int = 0,
                      wav_dev_ptr: Optional[int] = None, wav_stride: Optional[int] = None, reuse_output: bool = True,
                      sample_rate=None, encoding="f32", filter_width=None, speed=None, loudness=None, loudness_peak=LOUDNESS_PEAK_DEFAULT,
                      loudness_max_gain=LOUDNESS_MAX_GAIN_DEFAULT):
        """Codes already on the device (BackboneEngine.export_codes) -> waveforms, asynchronously: returns the [n, stride]
        destination (a view of the engine's pinned host buffer, or None when `wav_dev_ptr` names a device buffer);
        call sync() before reading it.  float32 at 24 kHz by default; with an output format (as `decode`) elements of the encoding's dtype,
        stride = wav_out_len(hop_length * max(lens), sample_rate) unless given, row i valid up to wav_out_len(hop_length * lens[i], sample_rate).
        With speed (as `decode`) the lengths are those of the stretched utterances; loudness / loudness_peak / loudness_max_gain as `decode`
        (ntts_codec_decode_dev_loud, the entry point of every call with a stage on)."""
        fmt = wav_format(sample_rate, encoding, filter_width)
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        n = len(lens)
        pm = speed_permille(speed, n)
        loud = loudness_params(loudness, loudness_peak, loudness_max_gain, n)
        stride = int(wav_stride or self._row_len(lens, fmt[0], pm))
        wav = None
        if wav_dev_ptr is None:
            wav = self._pinned(n * stride, fmt[1]).reshape(n, stride)
            dst, on_dev = wav.ctypes.data, 0
        else:
            dst, on_dev = wav_dev_ptr, 1
        self._decode_entry(n, codes_dev_ptr, lens, fmt, pm, loud, dst, stride, dev=(codes_stride, on_dev, producer_stream))
        return wav

    def sync(self):
        self._chk(self.lib.ntts_codec_sync(self.h))

    def set_stream(self, stream: Optional[int]):
        """Run the codec passes on the caller's HIP stream (a hipStream_t as an integer); None = the engine's own."""
        self._chk(self.lib.ntts_codec_set_stream(self.h, C.c_void_p(stream or None)))

    def last_timing(self) -> float:
        ms = C.c_float()
        self._chk(self.lib.ntts_codec_last_timing(self.h, C.byref(ms)))
        return ms.value


class WavStream:
    """The codec's output stage on `n` independent 24 kHz float32 signals that arrive in chunks (ntts_wav_stream_*): every stream keeps the
    few input samples its next outputs still need, and its chunks, concatenated, are CodecEngine.convert of the concatenated signal bit for
    bit.  A chunk's output lags its input by up to width + orig samples; `last` flushes a stream, which is then empty and may start again."""

    def __init__(self, codec: "CodecEngine", n: int = 1, sample_rate=None, encoding="f32", filter_width=None, max_chunk_samples: int = 16384):
        self.lib = codec.lib
        self.fmt, self.dtype, self.native = wav_format(sample_rate, encoding, filter_width)
        self.n, self.max_chunk_samples = int(n), int(max_chunk_samples)
        h = C.c_void_p()
        rc = self.lib.ntts_wav_stream_create(codec.h, C.byref(self.fmt), self.n, self.max_chunk_samples, C.byref(h))
        if rc != 0:
            raise NeuTTSHipError(rc, (self.lib.ntts_wav_stream_last_error(None) or b"").decode())
        self.h = h
        self._keep = codec                                               # the converter borrows the engine
        self._total = [0] * self.n                                       # input samples of every stream's current signal

    def _chk(self, rc: int):
        if rc != 0:
            raise NeuTTSHipError(rc, (self.lib.ntts_wav_stream_last_error(self.h) or b"").decode())

    def out_count(self, n_in_total: int, last: bool = False) -> int:
        """Output samples a stream has emitted in all after n_in_total input samples (ntts_wav_stream_count)."""
        m = C.c_int64()
        rc = self.lib.ntts_wav_stream_count(C.byref(self.fmt), int(n_in_total), int(bool(last)), C.byref(m))
        if rc != 0:
            raise NeuTTSHipError(rc, (self.lib.ntts_wav_stream_last_error(None) or b"").decode())
        return m.value

    def push_array(self, streams, wav: np.ndarray, n_samples, last, out_stride: Optional[int] = None):
        """One ntts_wav_stream_push: wav [k, in_stride] float32, row i = n_samples[i] new samples of stream streams[i] (its final chunk if
        last[i]) -> ([k, out_stride] array of the encoding's dtype, elements per row)."""
        wav = np.ascontiguousarray(wav, dtype=np.float32)
        k, in_stride = wav.shape
        st = np.ascontiguousarray(streams, dtype=np.int32)
        ns = np.ascontiguousarray(n_samples, dtype=np.int32)
        la = np.ascontiguousarray(np.asarray(last).astype(np.int32))
        if not (len(st) == len(ns) == len(la) == k):
            raise ValueError(f"streams / n_samples / last: {len(st)} / {len(ns)} / {len(la)} values for {k} rows")
        if out_stride is None:          # what the longest chunk of this call can emit, the stream's held-back outputs included
            out_stride = max([1] + [self.out_count(self._total[int(u)] + int(v), bool(f)) - self.out_count(self._total[int(u)])
                                    for u, v, f in zip(st, ns, la) if 0 <= int(u) < self.n and int(v) >= 0])
        out_stride = int(out_stride)
        buf = np.zeros(max(1, k * max(0, out_stride)), dtype=self.dtype)
        out_lens = np.zeros(k, dtype=np.int32)
        i32p = C.POINTER(C.c_int32)
        self._chk(self.lib.ntts_wav_stream_push(self.h, k, st.ctypes.data_as(i32p), wav.ctypes.data_as(C.POINTER(C.c_float)), in_stride,
                                                ns.ctypes.data_as(i32p), la.ctypes.data_as(i32p), C.c_void_p(buf.ctypes.data), out_stride,
                                                out_lens.ctypes.data_as(i32p)))
        for u, v, f in zip(st, ns, la):
            self._total[int(u)] = 0 if f else self._total[int(u)] + int(v)
        return buf[: k * out_stride].reshape(k, out_stride), out_lens

    def push(self, chunks: Sequence[np.ndarray], streams: Optional[Sequence[int]] = None, last=False) -> List[np.ndarray]:
        """chunks: one 1-D float32 array per entry, for streams `streams` (default 0, 1, ...); last: one flag or one per entry -> the chunks in
        the output format."""
        chunks = [np.asarray(c, dtype=np.float32).reshape(-1) for c in chunks]
        if not chunks:
            return []
        streams = list(range(len(chunks))) if streams is None else list(streams)
        last = [bool(last)] * len(chunks) if isinstance(last, (bool, np.bool_, int)) else [bool(f) for f in last]
        buf = np.zeros((len(chunks), max(1, max(len(c) for c in chunks))), dtype=np.float32)
        for r, c in enumerate(chunks):
            buf[r, : len(c)] = c
        out, out_lens = self.push_array(streams, buf, [len(c) for c in chunks], last)
        return [out[r, : int(out_lens[r])] for r in range(len(chunks))]

    def close(self):
        if getattr(self, "h", None):
            self.lib.ntts_wav_stream_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SpeedStream:
    """The codec's time stretch on `n` independent 24 kHz float32 signals that arrive in chunks, the output stage behind it (ntts_speed_stream_*):
    every stream keeps its last position and at most 1 560 input samples on the device, and its chunks, concatenated, are
    CodecEngine.stretch of the concatenated signal bit for bit.  A stream has one speed per signal; at a speed other than 1 a chunk's output lags
    its input by up to 960 samples (40 ms) and one frame, and may be empty; `last` flushes a stream, which is then empty and may start again at
    another speed."""

    def __init__(self, codec: "CodecEngine", n: int = 1, speed=1.0, sample_rate=None, encoding="f32", filter_width=None, max_chunk_samples: int = 16384):
        self.lib = codec.lib
        self.fmt, self.dtype, self.native = wav_format(sample_rate, encoding, filter_width)
        self.n, self.max_chunk_samples = int(n), int(max_chunk_samples)
        pm = speed_permille(speed, self.n)
        self.permille = np.full(self.n, 1000, dtype=np.int32) if pm is None else pm
        h = C.c_void_p()
        rc = self.lib.ntts_speed_stream_create(codec.h, C.byref(self.fmt), self.n, self.max_chunk_samples, C.byref(h))
        if rc != 0:
            raise NeuTTSHipError(rc, (self.lib.ntts_speed_stream_last_error(None) or b"").decode())
        self.h = h
        self._keep = codec                                               # the stretcher borrows the engine
        self._conv = WavStream.__new__(WavStream)                        # ntts_wav_stream_count of this format: host arithmetic, no handle
        self._conv.lib, self._conv.fmt = self.lib, self.fmt
        self._total = [0] * self.n                                       # input samples of every stream's current signal

    def _chk(self, rc: int):
        if rc != 0:
            raise NeuTTSHipError(rc, (self.lib.ntts_speed_stream_last_error(self.h) or b"").decode())

    def _emits(self, u: int, pm: int, v: int, last: bool):
        """(stretched samples, elements of the format) stream u emits for v more samples: the two stages' counts, one behind the other."""
        n0 = self._total[u]
        s0, s1 = self.out_count(n0, pm), self.out_count(n0 + v, pm, last)
        return s1 - s0, self._conv.out_count(s1, last) - self._conv.out_count(s0)

    def out_count(self, n_in_total: int, permille: int = 1000, last: bool = False) -> int:
        """24 kHz samples a stream at `permille` has emitted in all after n_in_total input samples (ntts_speed_stream_count)."""
        m = C.c_int64()
        rc = self.lib.ntts_speed_stream_count(int(permille), int(n_in_total), int(bool(last)), C.byref(m))
        if rc != 0:
            raise NeuTTSHipError(rc, (self.lib.ntts_speed_stream_last_error(None) or b"").decode())
        return m.value

    def push_array(self, streams, wav: np.ndarray, n_samples, last, permille=None, out_stride: Optional[int] = None, pos_stride: Optional[int] = None):
        """One ntts_speed_stream_push: wav [k, in_stride] float32, row i = n_samples[i] new samples of stream streams[i] (its final chunk if
        last[i]) at permille[i] (default: the stream's speed of the constructor) -> ([k, out_stride] array of the encoding's dtype, elements
        per row, [k, pos_stride] int32 positions decided in this call, positions per row)."""
        wav = np.ascontiguousarray(wav, dtype=np.float32)
        k, in_stride = wav.shape
        st = np.ascontiguousarray(streams, dtype=np.int32)
        ns = np.ascontiguousarray(n_samples, dtype=np.int32)
        la = np.ascontiguousarray(np.asarray(last).astype(np.int32))
        if permille is None:
            permille = [self.permille[int(u)] if 0 <= int(u) < self.n else 1000 for u in st]
        pm = np.ascontiguousarray(permille, dtype=np.int32)
        if not (len(st) == len(ns) == len(la) == len(pm) == k):
            raise ValueError(f"streams / n_samples / last / permille: {len(st)} / {len(ns)} / {len(la)} / {len(pm)} values for {k} rows")
        # what the longest chunk of this call emits through both stages, what they held back included
        ok = [(int(u), int(m), int(v), bool(f)) for u, m, v, f in zip(st, pm, ns, la)
              if 0 <= int(u) < self.n and int(v) >= 0 and SPEED_PERMILLE_MIN <= int(m) <= SPEED_PERMILLE_MAX]
        emits = [self._emits(*e) for e in ok]
        if out_stride is None:
            out_stride = max([1] + [e[1] for e in emits])
        if pos_stride is None:
            pos_stride = max([1] + [e[0] // STRETCH_HOP + 2 for e in emits])
        out_stride, pos_stride = int(out_stride), int(pos_stride)
        buf = np.zeros(max(1, k * max(0, out_stride)), dtype=self.dtype)
        pos = np.zeros(max(1, k * max(0, pos_stride)), dtype=np.int32)
        out_lens, n_pos = np.zeros(k, dtype=np.int32), np.zeros(k, dtype=np.int32)
        i32p = C.POINTER(C.c_int32)
        self._chk(self.lib.ntts_speed_stream_push(self.h, k, st.ctypes.data_as(i32p), pm.ctypes.data_as(i32p), wav.ctypes.data_as(C.POINTER(C.c_float)),
                                                  in_stride, ns.ctypes.data_as(i32p), la.ctypes.data_as(i32p), C.c_void_p(buf.ctypes.data), out_stride,
                                                  out_lens.ctypes.data_as(i32p), pos.ctypes.data_as(i32p), pos_stride, n_pos.ctypes.data_as(i32p)))
        for u, v, f in zip(st, ns, la):
            self._total[int(u)] = 0 if f else self._total[int(u)] + int(v)
        return buf[: k * out_stride].reshape(k, out_stride), out_lens, pos[: k * pos_stride].reshape(k, pos_stride), n_pos

    def push(self, chunks: Sequence[np.ndarray], streams: Optional[Sequence[int]] = None, last=False, speed=None) -> List[np.ndarray]:
        """chunks: one 1-D float32 array per entry, for streams `streams` (default 0, 1, ...); last: one flag or one per entry; speed: one value or
        one per entry (default: the constructor's) -> the chunks at that speed in the output format."""
        chunks = [np.asarray(c, dtype=np.float32).reshape(-1) for c in chunks]
        if not chunks:
            return []
        streams = list(range(len(chunks))) if streams is None else list(streams)
        last = [bool(last)] * len(chunks) if isinstance(last, (bool, np.bool_, int)) else [bool(f) for f in last]
        pm = None
        if speed is not None:
            pm = speed_permille(speed, len(chunks))
            pm = np.full(len(chunks), 1000, dtype=np.int32) if pm is None else pm
        buf = np.zeros((len(chunks), max(1, max(len(c) for c in chunks))), dtype=np.float32)
        for r, c in enumerate(chunks):
            buf[r, : len(c)] = c
        out, out_lens, _, _ = self.push_array(streams, buf, [len(c) for c in chunks], last, pm)
        return [out[r, : int(out_lens[r])] for r in range(len(chunks))]

    def close(self):
        if getattr(self, "h", None):
            self.lib.ntts_speed_stream_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class StreamSet:
    """Device-side streaming state of `n` concurrent infer_stream utterances (ntts_streams_*, ABI 6): token caches, window assembly,
    the 27-frame slice and the cross-fade with the previous chunk (ref:neutts/neutts.py:385-388, :401-465) run on the device; per burst
    the host sees a few integers per stream and receives each stream's new samples."""

    def __init__(self, backbone: "BackboneEngine", codec: "CodecEngine", slots: Sequence[int], ref_codes: Sequence[Sequence[int]],
                 max_new_tokens: int, chunk: int, lookforward: int, lookback: int, overlap: int, hop_length: int, speech_base: int,
                 n_codes: int, modulo: bool = False, fmt=None, speed=None):
        """fmt: None (24 kHz float32 chunks) or (sample_rate, encoding, filter_width): the chunked output stage behind the cross-fade.
        speed: None (all at 1.0), one value or one per stream: the chunked time stretch behind the cross-fade, ahead of the output stage."""
        self.lib = backbone.lib
        self.n = len(slots)
        prm = StreamParamsC(chunk, lookforward, lookback, overlap, hop_length, speech_base, n_codes, int(bool(modulo)))
        sl = np.ascontiguousarray(slots, dtype=np.int32)
        lens = np.array([len(r) for r in ref_codes], dtype=np.int32)
        flat = np.ascontiguousarray(np.concatenate([np.asarray(r, dtype=np.int32) for r in ref_codes]) if lens.sum() else np.zeros(1, np.int32))
        i32p = C.POINTER(C.c_int32)
        h = C.c_void_p()
        rc = self.lib.ntts_streams_create(backbone.h, codec.h, C.byref(prm), backbone._device, self.n, sl.ctypes.data_as(i32p),
                                          flat.ctypes.data_as(i32p), lens.ctypes.data_as(i32p), int(max_new_tokens), C.byref(h))
        if rc != 0:
            raise NeuTTSHipError(rc, (self.lib.ntts_streams_last_error(None) or b"").decode())
        self.h = h
        self._keep = (backbone, codec)                                   # the set borrows both engines
        cap = 2 * self.n
        self._cs, self._cn, self._cl = (np.zeros(cap, dtype=np.int32) for _ in range(3))
        self._fmt = None
        if fmt is not None:
            fc, dtype, native = wav_format(*fmt)
            if not native:                                               # (the native format spelled out: the calls of a set without one)
                self.set_format(fc)
                self._fmt = (fc, dtype)
        pm = speed_permille(speed, self.n)
        if pm is not None:                                               # (all at 1.0: the calls of a set without the stage)
            self.set_speed(pm)

    def set_speed(self, permille):
        """ntts_streams_set_speed as it is: int32 per mille per stream, or None for all 1000; legal until the first pump_begin."""
        pm = None if permille is None else np.ascontiguousarray(permille, dtype=np.int32)
        if pm is not None and len(pm) != self.n:
            raise ValueError(f"set_speed: {len(pm)} values for {self.n} streams")
        self._chk(self.lib.ntts_streams_set_speed(self.h, pm.ctypes.data_as(C.POINTER(C.c_int32)) if pm is not None else None))

    def set_format(self, fc: "WavFormatC"):
        """ntts_streams_set_format as it is: legal until the first pump_begin."""
        self._chk(self.lib.ntts_streams_set_format(self.h, C.byref(fc) if fc is not None else None))

    def _chk(self, rc: int):
        if rc != 0:
            raise NeuTTSHipError(rc, (self.lib.ntts_streams_last_error(self.h) or b"").decode())

    def pump_begin(self):
        """Append the ids generated so far to the caches and snapshot the streams behind the decode steps enqueued so far (async)."""
        self._chk(self.lib.ntts_streams_pump_begin(self.h))

    def pump_wait(self) -> int:
        """Wait for the snapshot of pump_begin alone; returns the number of streams still generating in it."""
        run = C.c_int32()
        self._chk(self.lib.ntts_streams_pump_wait(self.h, C.byref(run)))
        return run.value

    def pump_end(self):
        """-> (chunks, n_running, more): chunks = [(stream, samples (view of pinned memory, valid until the next pump_end), last)]; with an
        output format the samples are of its dtype (and a chunk may be empty)."""
        i32p = C.POINTER(C.c_int32)
        n, run, more = C.c_int32(), C.c_int32(), C.c_int32()
        if self._fmt is not None:
            dtype = np.dtype(self._fmt[1])
            vptr, stride = C.c_void_p(), C.c_int64()
            self._chk(self.lib.ntts_streams_pump_end_fmt(self.h, len(self._cs), C.byref(n), self._cs.ctypes.data_as(i32p), self._cn.ctypes.data_as(i32p),
                                                         self._cl.ctypes.data_as(i32p), C.byref(vptr), C.byref(stride), C.byref(run), C.byref(more)))
            out = []
            if n.value:
                nbytes = n.value * stride.value * dtype.itemsize
                buf = np.frombuffer((C.c_char * nbytes).from_address(vptr.value), dtype=dtype).reshape(n.value, stride.value)
                out = [(int(self._cs[k]), buf[k, : int(self._cn[k])], bool(self._cl[k])) for k in range(n.value)]
            return out, run.value, bool(more.value)
        ptr, stride = C.POINTER(C.c_float)(), C.c_int64()
        self._chk(self.lib.ntts_streams_pump_end(self.h, len(self._cs), C.byref(n), self._cs.ctypes.data_as(i32p), self._cn.ctypes.data_as(i32p),
                                                 self._cl.ctypes.data_as(i32p), C.byref(ptr), C.byref(stride), C.byref(run), C.byref(more)))
        out = []
        if n.value:
            buf = np.ctypeslib.as_array(ptr, shape=(n.value, stride.value))
            out = [(int(self._cs[k]), buf[k, : int(self._cn[k])], bool(self._cl[k])) for k in range(n.value)]
        return out, run.value, bool(more.value)

    def done(self) -> int:
        d = C.c_int32()
        self._chk(self.lib.ntts_streams_done(self.h, C.byref(d)))
        return d.value

    def close(self):
        if getattr(self, "h", None):
            self.lib.ntts_streams_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class EncoderEngine:
    """NeuCodec encoder on one GPU: 16 kHz mono waveform -> FSQ codes at 50 Hz (replaces codec.encode_code,
    ref:neutts/neutts.py:266-271).  One clip per call; fp32."""

    STAGES = {"features": 0, "concat": 1, "fc": 2, "latents": 3}

    def __init__(self, cfg: dict, device: int = 0, lib_path: Optional[str] = None):
        self.lib = load_library(lib_path)
        ratios = list(cfg.get("ratios", [2, 2, 4, 4, 5]))
        lv = list(cfg.get("levels", [4] * 8))
        self.hop = int(np.prod(ratios))
        self.max_samples = int(cfg.get("max_samples", 30 * 16000))
        c = EncoderConfigC(cfg.get("sem_hidden", 1024), cfg.get("sem_layers", 16), cfg.get("sem_heads", 16),
                           cfg.get("sem_ffn", 4096), cfg.get("sem_conv_kernel", 31), cfg.get("sem_left", 64),
                           cfg.get("sem_right", 8), cfg.get("sem_ln_eps", 1e-5), cfg.get("ac_hidden", 48), len(ratios),
                           (C.c_int32 * 8)(*(ratios + [1] * (8 - len(ratios)))), cfg.get("codec_hidden", 1024), len(lv),
                           (C.c_int32 * 8)(*(lv + [1] * (8 - len(lv)))), self.max_samples)
        h = C.c_void_p()
        rc = self.lib.ntts_encoder_create(C.byref(c), device, C.byref(h))
        if rc != 0:
            raise NeuTTSHipError(rc, (self.lib.ntts_encoder_last_error(None) or b"").decode())
        self.h = h
        self.device = device

    def _chk(self, rc: int):
        if rc != 0:
            raise NeuTTSHipError(rc, (self.lib.ntts_encoder_last_error(self.h) or b"").decode())

    def close(self):
        if getattr(self, "h", None):
            self.lib.ntts_encoder_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load_state_dict(self, sd: Dict[str, object]):
        """Encoder tensors of an Xcodec2Model-named state dict; decoder / project_out entries are skipped here (they belong
        to CodecEngine), anything else unknown is an error at finalize only if a needed tensor is missing."""
        for k, v in sd.items():
            if k.startswith(("acoustic_decoder.", "decoder.", "quantizer.project_out.")) or k.endswith("masked_spec_embed"):
                continue
            ptr, code, shape, is_dev, keep = _tensor_ptr(v)
            shp = (C.c_int64 * len(shape))(*shape)
            self._chk(self.lib.ntts_encoder_load_tensor(self.h, k.encode(), C.c_void_p(ptr), code, shp, len(shape), is_dev))
            del keep
        self._chk(self.lib.ntts_encoder_finalize(self.h))

    def encode(self, wav: np.ndarray) -> np.ndarray:
        """wav: float32 mono at 16 kHz, [L] -> int32 codes [L // hop + 1]."""
        w = np.ascontiguousarray(np.asarray(wav, dtype=np.float32).reshape(-1))
        if w.size < 1:
            raise ValueError("empty waveform")
        if w.size > self.max_samples:
            raise ValueError(f"clip of {w.size} samples exceeds max_samples {self.max_samples}")
        cap = w.size // self.hop + 2
        out = np.empty(cap, dtype=np.int32)
        n = C.c_int32()
        self._chk(self.lib.ntts_encoder_encode(self.h, w.ctypes.data_as(C.POINTER(C.c_float)), w.size,
                                               out.ctypes.data_as(C.POINTER(C.c_int32)), cap, C.byref(n)))
        return out[: n.value].copy()

    def read_stage(self, name: str) -> np.ndarray:
        """Intermediate of the last encode() call ('features' | 'concat' | 'fc' | 'latents') as [T, C] float32."""
        cap = (self.max_samples // self.hop + 2) * 4096
        buf = np.empty(cap, dtype=np.float32)
        r, c = C.c_int32(), C.c_int32()
        self._chk(self.lib.ntts_encoder_read_stage(self.h, self.STAGES[name], buf.ctypes.data_as(C.POINTER(C.c_float)), cap,
                                                   C.byref(r), C.byref(c)))
        return buf[: r.value * c.value].reshape(r.value, c.value).copy()

    def last_timing(self) -> float:
        ms = C.c_float()
        self._chk(self.lib.ntts_encoder_last_timing(self.h, C.byref(ms)))
        return ms.value

