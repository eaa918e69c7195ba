"""NeuTTS -- the reference's class surface (ref:neutts/neutts.py:73-465) over the MI355X-native hot path.

Same constructor arguments, public attributes, `infer` / `infer_stream` / `encode_reference` signatures, return
types and error messages as the reference; the two third-party calls on its hot path are replaced:

    self.backbone.generate(...)      ref:neutts/neutts.py:338-347   ->  _hip.BackboneEngine (HIP, paged KV, batched)
    self.codec.decode_code(codes)    ref:neutts/neutts.py:288-291   ->  _hip.CodecEngine    (HIP)

and the id -> string -> regex -> id round trip between them (ref :349 -> :276) becomes `code = id - id(<|speech_0|>)`
with a range mask (ids outside the speech range are dropped, exactly what the regex does).

Differences, all deliberate:
  * devices: this implementation runs on MI355X only -- "cpu" raises (there is no CPU fallback); defaults are "cuda".
  * `infer_stream` is implemented for this backend (the reference raises NotImplementedError for torch, :264) with
    the GGUF path's window / overlap-add semantics (:401-465).
  * batched entry points (`infer_batch`, `infer_stream_batch`, `generate_codes`, `decode_codes`) expose what the engine is
    built for.
  * GGUF (llama.cpp) backbones and the ONNX codec are other runtimes of the same model and are not provided.
Optional front/back-end dependencies (phonemizer, librosa, neucodec, perth) are imported lazily, where used.
"""
from __future__ import annotations

import re
import warnings
from pathlib import Path
from typing import Dict, Generator, List, Optional, Sequence

import numpy as np

from . import _hip

_SPEECH_RE = re.compile(r"<\|speech_(\d+)\|>")


def _linear_overlap_add(frames: List[np.ndarray], stride: int) -> np.ndarray:
    """Triangular-weight cross-fade of overlapping chunks; behaviour of ref:neutts/neutts.py:46-70."""
    assert len(frames)
    dtype = frames[0].dtype
    total = max(stride * i + f.shape[-1] for i, f in enumerate(frames))
    weight_sum = np.zeros(total, dtype=dtype)
    mixed = np.zeros(total, dtype=dtype)
    for i, f in enumerate(frames):
        n = f.shape[-1]
        t = np.linspace(0, 1, n + 2, dtype=dtype)[1:-1]
        tri = np.abs(0.5 - (t - 0.5))
        mixed[stride * i: stride * i + n] += tri * f
        weight_sum[stride * i: stride * i + n] += tri
    assert weight_sum.min() > 0
    return mixed / weight_sum


class _StreamBlender:
    """Incremental form of the reference's streaming post-process (ref:neutts/neutts.py:441-448, :461-465): the
    reference re-blends its whole audio cache for every chunk (O(n^2)); frames are `chunk + 2*overlap` hops long at a
    stride of `chunk` hops, so only the previous frame can touch the samples a new frame releases.  `push` returns
    exactly `_linear_overlap_add(all frames)[n_decoded_samples:new_end]` (bit-identical: same operands, same order)."""

    def __init__(self, stride: int):
        self.stride = stride
        self.prev: Optional[np.ndarray] = None

    def push(self, frame: np.ndarray, last: bool = False) -> np.ndarray:
        st = self.stride
        if self.prev is None:
            mixed = _linear_overlap_add([frame], stride=st)
            out = mixed if last else mixed[:st]
        else:
            assert self.prev.shape[-1] < 2 * st, "frame longer than two strides: more than one frame overlaps"
            mixed = _linear_overlap_add([self.prev, frame], stride=st)
            out = mixed[st:] if last else mixed[st:2 * st]
        self.prev = frame
        return out


def _device_index(device, what: str) -> int:
    s = str(device)
    if s in ("gpu", "cuda", "hip"):
        return 0
    if s.startswith("cuda:") or s.startswith("hip:"):
        return int(s.split(":", 1)[1])
    raise RuntimeError(
        f"{what}={device!r}: this NeuTTS implementation runs on AMD MI355X (gfx950) only and has no CPU fallback; "
        "pass 'cuda' / 'cuda:N'.")


class _CodecFacade:
    """What `self.codec` looks like to callers of the reference: `.decode_code(codes[B,1,T]) -> wav[B,1,480*T]`,
    `.encode_code(audio_or_path=...) -> codes[B,1,T]` and `.device`.  `enc_engine` = the on-device encoder
    (_hip.EncoderEngine), the only encoder there is: no torch module is kept beside it."""

    def __init__(self, engine: _hip.CodecEngine, enc_engine: Optional[_hip.EncoderEngine] = None):
        self.engine = engine
        self.enc_engine = enc_engine
        self.device = f"cuda:{engine.device}"

    def decode_code(self, codes):
        arr = np.asarray(codes.cpu() if hasattr(codes, "cpu") else codes)
        if arr.ndim != 3 or arr.shape[1] != 1:
            raise ValueError("codes must have shape [B, 1, T]")
        wavs = self.engine.decode([arr[b, 0].tolist() for b in range(arr.shape[0])])
        import torch  # tensor container for API compatibility
        return torch.from_numpy(np.stack(wavs)[:, None, :])

    def encode_code(self, audio_or_path):
        """neucodec `encode_code`: a path, or a 16 kHz waveform [B, 1, L] (tensor / array) -> int codes [B, 1, T]."""
        if self.enc_engine is None:
            raise RuntimeError("Reference encoding needs encoder weights on the encoder engine: a codec spec with an 'encoder' entry "
                               "or a NeuCodec checkpoint; or pre-encode references (ref:examples/encode_reference.py).")
        import torch  # tensor container for API compatibility
        if isinstance(audio_or_path, (str, Path)):
            wavs = [load_audio_16k(audio_or_path)]
        else:
            arr = np.asarray(audio_or_path.detach().cpu() if hasattr(audio_or_path, "detach") else audio_or_path, dtype=np.float32)
            if arr.ndim == 1:
                arr = arr[None, None, :]
            elif arr.ndim == 2:
                arr = arr[:, None, :]
            if arr.ndim != 3 or arr.shape[1] != 1:
                raise ValueError("audio must have shape [B, 1, L] (mono, 16 kHz)")
            wavs = [arr[b, 0] for b in range(arr.shape[0])]
        return torch.from_numpy(np.stack([self.enc_engine.encode(w) for w in wavs])[:, None, :].astype(np.int64))


def load_audio_16k(path) -> np.ndarray:
    """`librosa.load(path, sr=16000, mono=True)` (ref:neutts/neutts.py:268) -> float32 [L].  Without librosa, PCM / float WAV
    files are read with scipy and resampled with a polyphase filter (a front-end detail: the two resamplers are not
    sample-identical); anything else needs librosa, as in the reference."""
    try:
        import librosa
    except ImportError:
        librosa = None
    if librosa is not None:
        wav, _ = librosa.load(str(path), sr=16000, mono=True)
        return np.asarray(wav, dtype=np.float32)
    if not str(path).lower().endswith(".wav"):
        raise ImportError("Reading this audio format needs librosa (pip install librosa), as in the reference.")
    from math import gcd
    from scipy.io import wavfile
    from scipy.signal import resample_poly
    sr, x = wavfile.read(str(path))
    if x.dtype.kind == "i":
        x = x.astype(np.float32) / float(2 ** (8 * x.dtype.itemsize - 1))
    elif x.dtype.kind == "u":
        x = (x.astype(np.float32) - 128.0) / 128.0
    x = x.astype(np.float32)
    if x.ndim == 2:
        x = x.mean(axis=1)
    if sr != 16000:
        g = gcd(int(sr), 16000)
        x = resample_poly(x, 16000 // g, int(sr) // g).astype(np.float32)
    return x


def _check_sampling(top_k, temperature, top_p, min_p, who: str = "") -> None:
    """The ranges transformers' warpers accept (TopK / Temperature / TopP / MinPLogitsWarper); ValueError before anything reaches the engine."""
    if isinstance(top_k, bool) or not isinstance(top_k, (int, np.integer)) or (top_k < 1 and top_k != _hip.TOP_K_OFF):
        raise ValueError(f"{who}top_k must be an integer >= 1, or -1 for the whole vocabulary (got {top_k!r})")
    for name, v in (("temperature", temperature), ("top_p", top_p), ("min_p", min_p)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError(f"{who}{name} must be a number (got {v!r})")
    if not temperature > 0 or temperature == float("inf"):
        raise ValueError(f"{who}temperature must be a finite number > 0 (got {temperature!r})")
    if not 0 < top_p <= 1:
        raise ValueError(f"{who}top_p must lie in (0, 1] (got {top_p!r})")
    if not 0 <= min_p <= 1:
        raise ValueError(f"{who}min_p must lie in [0, 1] (got {min_p!r})")


def _check_repetition(repetition_penalty, repetition_ignore_prompt, who: str = "") -> None:
    """RepetitionPenaltyLogitsProcessor's range (a strictly positive, finite float; 1.0 = off) and a plain bool; ValueError before anything
    reaches the engine."""
    v = repetition_penalty
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not v > 0 or v == float("inf"):
        raise ValueError(f"{who}repetition_penalty must be a finite number > 0 (got {v!r})")
    if not isinstance(repetition_ignore_prompt, (bool, np.bool_)):
        raise ValueError(f"{who}repetition_ignore_prompt must be True or False (got {repetition_ignore_prompt!r})")


def _check_best_of(best_of, do_sample: bool, who: str = "") -> None:
    """best_of: a plain integer >= 1; more than one candidate needs sampling (greedy candidates are all the same).  ValueError before anything
    reaches the engine."""
    if isinstance(best_of, (bool, np.bool_)) or not isinstance(best_of, (int, np.integer)) or best_of < 1:
        raise ValueError(f"{who}best_of must be an integer >= 1 (got {best_of!r})")
    if best_of > 1 and not do_sample:
        raise ValueError(f"{who}best_of = {best_of} needs do_sample=True: greedy candidates are identical")


def _check_output(sample_rate, encoding, filter_width, who: str = "") -> None:
    """The output formats the codec's device output stage produces (_hip.wav_format: include/neutts_hip.h ntts_wav_format); ValueError naming the
    offending value before anything reaches the engine."""
    _hip.wav_format(sample_rate, encoding, filter_width, who)


_INSTANCE_FORMAT = object()      # "the instance's stream_* attributes" as a default argument (None is the native format)
_INSTANCE = object()             # "the instance's loudness" as a default argument (None switches the option off)


def sequence_score(logprobs) -> float:
    """A candidate's score: the arithmetic mean of its per-token log-probabilities (-inf for an empty one)."""
    lp = np.asarray(logprobs, dtype=np.float64)
    return float(lp.mean()) if lp.size else float("-inf")


class NeuTTS:

    def __init__(
        self,
        backbone_repo="neuphonic/neutts-nano",
        backbone_device="cuda",
        codec_repo="neuphonic/neucodec",
        codec_device="cuda",
        *,
        max_batch: int = 1,
        engines: int = 1,
        lib_path: Optional[str] = None,
        do_sample: bool = True,
        seed: int = 0,
        top_k: int = 50,
        temperature: float = 1.0,
        top_p: float = 1.0,
        min_p: float = 0.0,
        repetition_penalty: float = 1.0,
        repetition_ignore_prompt: bool = False,
        logprobs: bool = False,
        best_of: int = 1,
        speech_range_head: bool = False,
        codec_precision: str = "fp16",
        output_sample_rate: int = 24_000,
        output_encoding: str = "f32",
        output_filter_width: int = 6,
        stream_sample_rate: int = 24_000,
        stream_encoding: str = "f32",
        stream_filter_width: Optional[int] = None,
        speed: float = 1.0,
        stream_speed: float = 1.0,
        loudness: Optional[float] = None,
        loudness_peak: float = -1.0,
        loudness_max_gain: float = 20.0,
    ):
        # Consts (ref:neutts/neutts.py:84-91)
        self.sample_rate = 24_000            # the NATIVE rate (the codec's; what a watermarker sees), whatever the output format
        # Output format of infer / infer_batch / decode_codes (the reference hands out 24 kHz float32, ref:neutts/neutts.py:288-291, and its users
        # resample and cast on the host): one of _hip.WAV_RATES, "f32" / "pcm16" (int16) / "mulaw" (uint8, G.711), the resampler's
        # lowpass_filter_width (torchaudio's default 6 rolls off early: telephony callers want 16 or more).  Applied on the device behind the codec
        # pass (include/neutts_hip.h ntts_wav_format); sample_rate= / encoding= per call override the first two.
        _check_output(output_sample_rate, output_encoding, output_filter_width, "output_")
        self.output_sample_rate = int(output_sample_rate)
        self.output_encoding = output_encoding
        self.output_filter_width = int(output_filter_width)
        # Format of the chunks of infer_stream / infer_stream_batch: a property of the transport, apart from the one above (a server hands mu-law
        # to its phone legs and keeps float files from infer).  The same stage with one history row of at most taps - 1 samples per stream
        # (ntts_streams_set_format / ntts_wav_stream_*): a stream's chunks, concatenated, are the one-shot stage's output of its concatenated
        # 24 kHz chunks bit for bit; they lag the native ones by up to width + orig input samples (under 10 ms).  stream_filter_width None =
        # output_filter_width.  stream_sample_rate= / stream_encoding= / stream_filter_width= per call override them.
        _check_output(stream_sample_rate, stream_encoding, output_filter_width if stream_filter_width is None else stream_filter_width, "stream_")
        self.stream_sample_rate = int(stream_sample_rate)
        self.stream_encoding = stream_encoding
        self.stream_filter_width = None if stream_filter_width is None else int(stream_filter_width)
        # How fast the voice speaks, 0.5 .. 2.0 (a codec-token model has no duration input: the reference offers nothing, its users resample, which
        # moves the pitch).  A pitch-preserving time stretch (WSOLA) on the device between the codec pass and the output stage (include/neutts_hip.h
        # ntts_codec_decode_speed): an utterance takes ceil(samples / speed) samples at 24 kHz.  speed= per call overrides it, one value or one per
        # utterance; the stream entry points take 1.0 only: their speed is stream_speed.
        _hip.speed_permille(speed, 1)
        self.speed = float(speed)
        # Speed of the chunks of infer_stream / infer_stream_batch, apart from the one above as the stream format is: the same stretch on chunks, with
        # each stream's state and at most 1 560 samples of history on the device (ntts_streams_set_speed / ntts_speed_stream_*), ahead of the chunks'
        # output format.  A stream's chunks, concatenated, are the one-shot stage's output of its concatenated speed-1 chunks bit for bit; at a speed
        # other than 1 they lag by up to 960 input samples (40 ms) and one frame -- the first audio comes that much later, only the last chunk is
        # longer for it, and a chunk may be empty.  stream_speed= per call overrides it, one value or one per utterance.
        _hip.speed_permille(stream_speed, 1, "stream_")
        self.stream_speed = float(stream_speed)
        # How loud an utterance comes out: a target in LUFS (-70 .. 0; None = as the codec gives it, which is about as loud as the reference clip
        # was -- the reference offers nothing, its users normalise on the host).  ITU-R BS.1770-4 integrated loudness (K-weighting, gating) measured
        # on the device at 24 kHz behind the time stretch and ahead of the output stage, then one gain per utterance (include/neutts_hip.h
        # ntts_codec_decode_loud): never more than loudness_max_gain dB, and never lifting the SAMPLE peak (not the true, inter-sample peak) above
        # loudness_peak dBFS.  loudness= per call overrides the target, one value or one per utterance (None = off).  A stream's gain is not known
        # before its end: the stream entry points refuse the option.
        _hip.loudness_params(-23.0 if loudness is None else loudness, loudness_peak, loudness_max_gain, 1, "instance ")
        self.loudness = None if loudness is None else float(loudness)
        self.loudness_peak = float(loudness_peak)
        self.loudness_max_gain = float(loudness_max_gain)
        self.max_context = 2048
        self.hop_length = 480
        self.streaming_overlap_frames = 1
        self.streaming_frames_per_chunk = 25
        self.streaming_lookforward = 5
        self.streaming_lookback = 50
        self.streaming_stride_samples = self.streaming_frames_per_chunk * self.hop_length
        self.streaming_overlap_compute = True    # backbone decode of chunk k+1 runs beside the codec pass of chunk k

        self._is_quantized_model = False
        self._is_onnx_codec = False
        self._lib_path = lib_path
        self._max_batch = max_batch
        # sampling contract of the reference call (ref:neutts/neutts.py:338-347: top_k 50, temperature 1.0 -- the defaults); do_sample=False = greedy.
        # top_p / min_p are generate()'s own keyword arguments of those names (TopPLogitsWarper / MinPLogitsWarper behind top-k), off in that
        # call.  Every entry point takes per-call overrides of the four.
        # repetition_penalty is generate()'s keyword argument of that name (RepetitionPenaltyLogitsProcessor, ahead of every warper; 1.0 = off, the
        # reference's value): codec-token decoders loop, and a penalty on tokens already seen is the standard remedy.  repetition_ignore_prompt = True
        # counts generated tokens only (the processor's prompt_ignore_length = the utterance's own prompt length): a cloning prompt is mostly
        # reference codec tokens.  Both have per-call overrides too.
        _check_sampling(top_k, temperature, top_p, min_p)
        _check_repetition(repetition_penalty, repetition_ignore_prompt)
        # logprobs=True keeps the engines' per-token log-probability record on (BackboneEngine.set_logprobs: log softmax of the processed logits row
        # at every chosen token, reduced inside the lm_head); an instance built without it switches it on for the calls that ask for scores and off
        # again.  best_of=N draws N candidates per utterance (one generate call, shared prompt pages) and keeps the one whose mean log-probability
        # is highest; return_logprobs= / return_scores= / best_of= per call on generate_codes / infer / infer_batch.
        if not isinstance(logprobs, (bool, np.bool_)):
            raise ValueError(f"logprobs must be True or False (got {logprobs!r})")
        _check_best_of(best_of, do_sample)
        self.logprobs = bool(logprobs)
        self.best_of = int(best_of)
        self.repetition_penalty = repetition_penalty
        self.repetition_ignore_prompt = repetition_ignore_prompt
        self.do_sample = do_sample
        self.top_k = top_k
        self.temperature = temperature
        self.top_p = top_p
        self.min_p = min_p
        self.min_new_tokens = 50
        self._seed = seed

        # NeuCodec's GEMM operand format (the reference runs this decoder in fp32, ref:neutts/neutts.py:288-291): "fp16" (default) = IEEE-half
        # operands, ~9.5e-4 RELATIVE rms of the fp32 decoder (8.1e-4 from the GEMM operands, the rest from the single-term fp16 ISTFT) -- inside BASELINE's 1e-3 absolute at any amplitude; "high" = split bf16 operands
        # (hi + lo), ~7e-4 at 3x the matrix-core work and bf16's range; "bf16" = rounds 1-5's default, 7e-3 relative
        if codec_precision not in ("fp16", "bf16", "high"):
            raise ValueError("codec_precision must be 'fp16', 'bf16' or 'high'")
        self._codec_precision = codec_precision
        self.tokenizer = None
        self.phonemizer = None       # created on first use: text front-end is off the hot path
        self._load_backbone(backbone_repo, backbone_device)
        self._load_codec(codec_repo, codec_device)
        # engines > 1 (serving; the reference runs one utterance at a time): that many backbone engines of `max_batch` slots each on
        # ONE copy of the weights, their decode chains side by side on the GPU (neutts._hip.EngineGang) -- infer_batch deals its
        # utterances out over them.  infer / infer_stream stay on the first engine.
        # speech_range_head=True (OPT-IN, off by default; SURVEY 7 "hard parts"): the lm_head over `<|speech_0|>` ... `<|speech_65535|>` +
        # `<|SPEECH_GENERATION_END|>` only -- the ids ref:neutts/neutts.py:276,336-341 can do anything with -- a third of the head's
        # bytes per decode step.  The reference samples over the whole vocabulary: the ids are its ids only while its choice lies in
        # that range (a trained checkpoint after a well-formed prompt), so this is a serving option, not the parity configuration.
        if speech_range_head:
            if self._speech_base is None or self._eos_id is None:
                raise RuntimeError("speech_range_head needs the ids of <|speech_0|> and <|SPEECH_GENERATION_END|> (tokenizer, or 'speech_base' / 'eos_token_id' with in-memory weights)")
            self.backbone.set_logits_range(int(self._speech_base), int(self._speech_base) + 65536, int(self._eos_id))
        self.gang = _hip.EngineGang(self.backbone, engines) if engines > 1 else None
        if self.logprobs:
            for eng in self._backbone_engines():
                eng.set_logprobs(True)

        try:  # optional watermarker, as the reference (ref:neutts/neutts.py:110-121)
            import perth
            self.watermarker = perth.PerthImplicitWatermarker()
        except (ImportError, AttributeError) as e:
            warnings.warn(f"Perth watermarking unavailable: {e}. Audio will not be watermarked. "
                          "Install with: pip install perth>=0.2.0")
            self.watermarker = None

    # ------------------------------------------------------------------------------------------ loading
    def close(self):
        """Release the GPU engines (not part of the reference's surface: its torch modules go with the garbage collector).  The gang
        goes first -- its twins read the first engine's arena and its lane streams carry engine 0's work."""
        gang, self.gang = getattr(self, "gang", None), None
        codecs, self._gang_codecs = getattr(self, "_gang_codecs", None), None
        for k, c in enumerate(codecs or []):
            c.set_stream(None)                       # (they ran on the gang's lanes)
            if k > 0:
                c.close()
        if gang is not None:
            gang.close()
        for name in ("backbone",):
            eng = getattr(self, name, None)
            if eng is not None and hasattr(eng, "close"):
                eng.close()
        codec = getattr(self, "codec", None)             # the class's own codec engine (gang codec 0) and the encoder engine: their GPU buffers and
        for eng in (getattr(codec, "engine", None), getattr(codec, "enc_engine", None)):   # page-locked staging rings do not wait for the collector
            if eng is not None and hasattr(eng, "close"):
                eng.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _load_backbone(self, backbone_repo, backbone_device):
        print(f"Loading backbone from: {backbone_repo if isinstance(backbone_repo, str) else '<in-memory weights>'}"
              f" on {backbone_device} ...")
        dev = _device_index(backbone_device, "backbone_device")
        if isinstance(backbone_repo, dict):
            # in-memory weights (tests, synthetic benchmarks): {"config", "state_dict", "inv_freq", "tokenizer",
            # "speech_base", "eos_token_id"}
            spec = backbone_repo
            cfg, sd, inv_freq = dict(spec["config"]), spec["state_dict"], spec["inv_freq"]
            input_scales = spec.get("input_scales")          # fp8 model (config["weight_dtype"] = "fp8"): static activation scales
            self.tokenizer = spec.get("tokenizer")
            self._speech_base = spec.get("speech_base")
            self._eos_id = spec.get("eos_token_id")
        else:
            if str(backbone_repo).endswith("gguf"):
                raise NotImplementedError(
                    "GGUF backbones run on llama.cpp (another runtime of the same model, quantised numerics); this "
                    "implementation provides the transformers-path backbone on MI355X only.")
            from transformers import AutoConfig, AutoModelForCausalLM, AutoTokenizer  # checkpoint readers only
            self.tokenizer = AutoTokenizer.from_pretrained(backbone_repo)
            hc = AutoConfig.from_pretrained(backbone_repo)
            cfg = _engine_config_from_hf(hc)
            input_scales = None
            sd = inv_freq = None
            shards = _safetensors_shards(backbone_repo)
            theta = _default_rope_theta(hc)
            if shards and theta is not None:
                # stream the checkpoint tensor by tensor into the engine's arena: no fp32 nn.Module copy of the model
                # on the host (the reference builds one, ref:neutts/neutts.py:164; only its weights matter here)
                import torch
                d = cfg["head_dim"]
                inv_freq = (1.0 / (theta ** (torch.arange(0, d, 2, dtype=torch.int64).to(dtype=torch.float) / d))).numpy()
                sd = _SafetensorsStateDict(shards)        # hf:modeling_rope_utils.py _compute_default_rope_parameters
                self._backbone_loader = "safetensors"
            else:
                model = AutoModelForCausalLM.from_pretrained(backbone_repo)
                sd = {k: v for k, v in model.state_dict().items() if not k.endswith("inv_freq")}
                inv_freq = model.model.rotary_emb.inv_freq.float().cpu().numpy()
                del model
                self._backbone_loader = "transformers"
            self._speech_base = self.tokenizer.convert_tokens_to_ids("<|speech_0|>")
            self._eos_id = self.tokenizer.convert_tokens_to_ids("<|SPEECH_GENERATION_END|>")
        cfg.setdefault("max_context", self.max_context)
        cfg["max_batch"] = self._max_batch
        cfg.setdefault("max_prefill_tokens", max(2 * self.max_context, 8192))
        self.backbone = _hip.BackboneEngine(cfg, dev, self._lib_path)
        self.backbone.load_state_dict(sd, inv_freq=inv_freq, input_scales=input_scales)
        self._vocab_size = cfg["vocab_size"]

    def _load_codec(self, codec_repo, codec_device):
        print(f"Loading codec from: {codec_repo if isinstance(codec_repo, str) else '<in-memory weights>'} on {codec_device} ...")
        dev = _device_index(codec_device, "codec_device")
        enc_spec = None
        if isinstance(codec_repo, dict):
            cfg, sd = dict(codec_repo["config"]), codec_repo["state_dict"]
            enc_spec = codec_repo.get("encoder")       # {"config": EncoderConfig fields, "state_dict": Xcodec2Model names}
        else:
            match codec_repo:
                case "neuphonic/neucodec" | "neuphonic/distill-neucodec":
                    try:
                        from neucodec import DistillNeuCodec, NeuCodec
                    except ImportError as e:
                        raise ImportError(
                            "Loading the NeuCodec checkpoint needs the `neucodec` package (weights + reference "
                            "encoder): pip install neucodec") from e
                    cls = NeuCodec if codec_repo == "neuphonic/neucodec" else DistillNeuCodec
                    # the package is the checkpoint READER only (its state dict is re-keyed and uploaded; the module is dropped):
                    # a tensor that does not map onto the engines is an error that lists the keys -- there is no torch fallback
                    full_sd = cls.from_pretrained(codec_repo).state_dict()
                    sd = neucodec_to_xcodec2_names(full_sd)
                    cfg = {}
                    enc_spec = {"config": {}, "state_dict": neucodec_encoder_to_xcodec2_names(full_sd)}
                case "neuphonic/neucodec-onnx-decoder":
                    raise NotImplementedError("The ONNX decoder is a CPU runtime of the same decoder; use "
                                              "'neuphonic/neucodec' for the MI355X path.")
                case _:
                    raise ValueError(
                        "Invalid codec repo! Must be one of:"
                        " 'neuphonic/neucodec', 'neuphonic/distill-neucodec',"
                        " 'neuphonic/neucodec-onnx-decoder'."
                    )
        cfg.setdefault("hop_length", self.hop_length)
        cfg.setdefault("precision", self._codec_precision)
        cfg.setdefault("max_frames", self.max_context)
        cfg.setdefault("max_rows", max(2 * (self.max_context + 6), self._max_batch * 512))
        self.hop_length = cfg["hop_length"]
        self.streaming_stride_samples = self.streaming_frames_per_chunk * self.hop_length
        engine = _hip.CodecEngine(cfg, dev, self._lib_path)
        engine.load_state_dict(sd)
        self._codec_spec = (dict(cfg), sd, dev)          # (a gang of stream sets gives every backbone engine a codec engine of its own)
        self._gang_codecs = None
        enc_engine = None
        if enc_spec is not None:
            ecfg = dict(enc_spec.get("config", {}))
            ecfg.setdefault("max_samples", 30 * 16000)       # the context holds ~30 s of audio (ref:README.md:35)
            enc_engine = _hip.EncoderEngine(ecfg, dev, self._lib_path)
            enc_engine.load_state_dict(enc_spec["state_dict"])
        self.codec = _CodecFacade(engine, enc_engine)

    # ------------------------------------------------------------------------------------------ public API
    def infer(self, text: str, ref_codes, ref_text: str, *, temperature=None, top_k=None, top_p=None, min_p=None, **repetition) -> np.ndarray:
        """Generate speech for `text` in the voice of the encoded reference (ref:neutts/neutts.py:216-243).  temperature / top_k / top_p /
        min_p override the instance's sampling attributes for this call (None = the attribute), and so do the two further keywords every entry
        point takes behind them: repetition_penalty= and repetition_ignore_prompt= (anything else is a TypeError).
        best_of=N: N sampled candidates, the one with the highest mean log-probability is synthesised; return_scores=True: (wav, score).
        sample_rate= / encoding= (two more keywords of the catch-all) override output_sample_rate / output_encoding for this call, speed= (0.5 .. 2.0)
        the instance's speed, loudness= (a target in LUFS; None = off) the instance's loudness."""
        out = self._resolve_output(repetition.pop("sample_rate", None), repetition.pop("encoding", None))
        speed = self._resolve_speed(repetition.pop("speed", None), 1)
        loud = self._resolve_loudness(repetition.pop("loudness", _INSTANCE), 1)
        best_of, want = self._pop_scoring(1, repetition, "return_scores")
        samp = self._resolve_sampling(1, temperature, top_k, top_p, min_p, repetition)
        prompt_ids = self._apply_chat_template(ref_codes, ref_text, text)
        ids, lps = self._generate_scored([prompt_ids], samp, best_of, want)
        if out is None and speed is None and loud is None:
            wav = self._decode_ids(ids[0])
            if self.watermarker is not None:
                wav = self.watermarker.apply_watermark(wav, sample_rate=24_000)
        else:
            speech_ids = self._ids_to_codes(ids[0])
            if len(speech_ids) == 0:
                raise ValueError("No valid speech tokens found in the output.")
            wav = self._decode_formatted([speech_ids], out, speed, loud)[0]
        return (wav, sequence_score(lps[0])) if want else wav

    def infer_batch(self, texts: Sequence[str], ref_codes, ref_texts, *, temperature=None, top_k=None, top_p=None, min_p=None, **repetition) -> List[np.ndarray]:
        """Many utterances at once: continuous batching over the engine's decode slots (over every engine's, with engines > 1),
        one codec pass.  The sampling overrides take one value for the call or one per utterance, and so does best_of= (candidates per
        utterance; only the winners go through the codec); return_scores=True: (wavs, scores), score = mean log-probability of the ids.
        sample_rate= / encoding= (two more keywords of the catch-all) override output_sample_rate / output_encoding for this call (one format per call),
        speed= the instance's speed: one value, or one per utterance; loudness= the instance's loudness target in the same way (None, or a None
        entry, = off)."""
        out = self._resolve_output(repetition.pop("sample_rate", None), repetition.pop("encoding", None))
        speed = self._resolve_speed(repetition.pop("speed", None), len(texts))
        loud = self._resolve_loudness(repetition.pop("loudness", _INSTANCE), len(texts))
        best_of, want = self._pop_scoring(len(texts), repetition, "return_scores")
        samp = self._resolve_sampling(len(texts), temperature, top_k, top_p, min_p, repetition)
        if not isinstance(ref_texts, (list, tuple)):
            ref_texts = [ref_texts] * len(texts)
            ref_codes = [ref_codes] * len(texts)
        prompts = [self._apply_chat_template(rc, rt, t) for rc, rt, t in zip(ref_codes, ref_texts, texts)]
        ids, lps = self._generate_scored(prompts, samp, best_of, want)
        codes = [self._ids_to_codes(x) for x in ids]
        if any(len(c) == 0 for c in codes):
            raise ValueError("No valid speech tokens found in the output.")
        if out is None and speed is None and loud is None:
            wavs = self.codec.engine.decode(codes)
            if self.watermarker is not None:
                wavs = [self.watermarker.apply_watermark(w, sample_rate=24_000) for w in wavs]
        else:
            wavs = self._decode_formatted(codes, out, speed, loud)
        return (wavs, [sequence_score(lp) for lp in lps]) if want else wavs

    def infer_stream(self, text: str, ref_codes, ref_text: str, *, temperature=None, top_k=None, top_p=None, min_p=None, **repetition) -> Generator[np.ndarray, None, None]:
        """Streaming synthesis with the reference's window / cross-fade semantics (ref:neutts/neutts.py:373-465).  Sampling overrides as `infer`
        (checked here, before the generator is handed out).  Chunks are 24 kHz float32 unless stream_sample_rate= / stream_encoding= /
        stream_filter_width= (or the instance's stream_* attributes) say otherwise; sample_rate= / encoding= / a non-native output_* attribute
        stay a ValueError here.  stream_speed= (or the instance's stream_speed) is the speed of this stream, 0.5 .. 2.0: the time stretch on its
        chunks, ahead of their format; the chunks then lag by up to 40 ms and a frame and may be empty.  speed= other than 1 stays a ValueError, and so
        does loudness= (or an instance whose loudness is set): an utterance's gain is known only at its end."""
        self._refuse_stream_output(repetition.pop("sample_rate", None), repetition.pop("encoding", None), "infer_stream")
        self._refuse_stream_speed(repetition.pop("speed", None), "infer_stream")
        self._refuse_stream_loudness(repetition.pop("loudness", _INSTANCE), "infer_stream")
        fmt = self._resolve_stream_output(repetition.pop("stream_sample_rate", None), repetition.pop("stream_encoding", None),
                                          repetition.pop("stream_filter_width", None))
        spd = self._resolve_stream_speed(repetition.pop("stream_speed", None), 1)
        samp = self._resolve_sampling(1, temperature, top_k, top_p, min_p, repetition)
        prompt_ids = self._apply_chat_template(ref_codes, ref_text, text)
        ref = [int(c) for c in _to_list(ref_codes)]
        if self._stream_on_device([ref]):       # token cache, windows, codec pass and cross-fade on the device (csrc/stream.cpp): a set of one stream
            return (chunk for _, chunk in self._infer_stream_batch_hip([prompt_ids], [ref], samp, fmt, spd))
        return self._infer_stream_hip(prompt_ids, ref, samp, fmt, spd)   # host loop: a watermarker (a host library) sits between the codec and the slice

    def infer_stream_batch(self, texts: Sequence[str], ref_codes, ref_texts, *, temperature=None, top_k=None, top_p=None, min_p=None, **repetition) -> Generator[tuple, None, None]:
        """Many utterances streamed at once (BASELINE config 5's shape: a decode batch with the codec on its own stream):
        yields `(utterance index, chunk)` pairs; the chunks of one utterance, in order, are exactly what `infer_stream`
        yields for it.  One decode burst serves every running utterance, and all windows that became decodable in a burst
        go through the codec in ONE batched call, enqueued behind the next burst (the two engines' streams overlap).
        At most `max_batch` utterances (the engine's decode slots) per call.  Sampling overrides as `infer_batch`.  Chunk format as
        `infer_stream`: stream_sample_rate= / stream_encoding= / stream_filter_width=, one format per call; stream_speed= one value or one per
        utterance."""
        self._refuse_stream_output(repetition.pop("sample_rate", None), repetition.pop("encoding", None), "infer_stream_batch")
        self._refuse_stream_speed(repetition.pop("speed", None), "infer_stream_batch")
        self._refuse_stream_loudness(repetition.pop("loudness", _INSTANCE), "infer_stream_batch")
        fmt = self._resolve_stream_output(repetition.pop("stream_sample_rate", None), repetition.pop("stream_encoding", None),
                                          repetition.pop("stream_filter_width", None))
        spd = self._resolve_stream_speed(repetition.pop("stream_speed", None), len(texts))
        samp = self._resolve_sampling(len(texts), temperature, top_k, top_p, min_p, repetition)
        if not isinstance(ref_texts, (list, tuple)):
            ref_texts = [ref_texts] * len(texts)
            ref_codes = [ref_codes] * len(texts)
        cap = self.gang.max_batch if (self.gang is not None and getattr(self, "stream_on_gang", False)) else self.backbone.max_batch
        if len(texts) > cap:
            raise ValueError(f"{len(texts)} utterances exceed the engine's {cap} decode slots")
        prompts = [self._apply_chat_template(rc, rt, t) for rc, rt, t in zip(ref_codes, ref_texts, texts)]
        return self._infer_stream_batch_hip(prompts, [[int(c) for c in _to_list(rc)] for rc in ref_codes], samp, fmt, spd)

    def score(self, text: str, codes, ref_codes, ref_text: str, include_eos: bool = True) -> Dict[str, object]:
        """Teacher-forced score of an EXISTING utterance: the model's log-probability of every speech token of `codes` (and, with include_eos, of
        `<|SPEECH_GENERATION_END|>` behind them) given the prompt `infer` would build for (text, ref_codes, ref_text) and the codes before it.
        No sampling setting and no logits processor enters (include/neutts_hip.h: ntts_backbone_score).  Returns dict(logprobs = float32 array,
        score = their mean as `sequence_score` computes it, top1_agreement = the fraction of positions where the model's argmax is the given
        token).  For filtering or ranking utterances, re-scoring candidates of another run, and comparing two builds on the same sequences."""
        return self.score_batch([text], [codes], ref_codes, ref_text, include_eos)[0]

    def score_batch(self, texts: Sequence[str], codes, ref_codes, ref_texts, include_eos: bool = True) -> List[Dict[str, object]]:
        """`score` for many utterances: one reference for all (ref_texts a string) or one per utterance, as `infer_batch` takes them.  The engine
        packs the sequences into as few prompt passes as its max_prefill_tokens and free decode slots allow; an utterance's values do not depend on
        what it is packed with.  RuntimeError on an instance with the restricted lm_head (speech_range_head=True): a score is over the whole vocabulary."""
        if not isinstance(include_eos, (bool, np.bool_)):
            raise ValueError(f"include_eos must be True or False (got {include_eos!r})")
        if getattr(self.backbone, "logits_range", None):
            raise RuntimeError("score needs the whole vocabulary: this instance runs the restricted lm_head (speech_range_head=True / set_logits_range); "
                               "build it without, or call backbone.set_logits_range(None) first")
        texts = list(texts)
        def as_list(c):      # (not _to_list: it would turn 2.5 or True into a code)
            if hasattr(c, "tolist"):
                a = np.asarray(c.cpu() if hasattr(c, "cpu") else c).reshape(-1)
                if a.dtype.kind not in "iu":
                    raise ValueError(f"codes must be integers (got dtype {a.dtype})")
                return a.tolist()
            return list(c)
        codes = [as_list(c) for c in codes]
        if len(codes) != len(texts):
            raise ValueError(f"codes: {len(codes)} sequences for {len(texts)} utterances")
        if not isinstance(ref_texts, (list, tuple)):
            ref_texts = [ref_texts] * len(texts)
            ref_codes = [ref_codes] * len(texts)
        if len(ref_texts) != len(texts) or len(ref_codes) != len(texts):
            raise ValueError(f"references: {len(ref_codes)} codes and {len(ref_texts)} texts for {len(texts)} utterances")
        who = lambda i: f"utterance {i}: " if len(texts) > 1 else ""
        for i, c in enumerate(codes):
            if len(c) == 0:
                raise ValueError(f"{who(i)}no codes to score")
            for v in c:
                if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not 0 <= v < 65536:
                    raise ValueError(f"{who(i)}codes must be integers in [0, 65536) (got {v!r})")
        if include_eos and self._eos_id is None:
            raise ValueError("include_eos needs the id of <|SPEECH_GENERATION_END|> (tokenizer, or 'eos_token_id' with in-memory weights)")
        seqs, froms = [], []
        for i, (t, c, rc, rt) in enumerate(zip(texts, codes, ref_codes, ref_texts)):
            prompt = self._apply_chat_template(rc, rt, t)
            ids = list(prompt) + self._codes_to_ids(c) + ([int(self._eos_id)] if include_eos else [])
            if max(ids) >= self.backbone.vocab_size or min(ids) < 0:
                raise ValueError(f"{who(i)}a code has no token in the model's vocabulary of {self.backbone.vocab_size}")
            if len(ids) > self.backbone.max_context:
                raise ValueError(f"{who(i)}prompt + codes are {len(ids)} tokens, the engine's max_context is {self.backbone.max_context}")
            seqs.append(ids)
            froms.append(len(prompt))
        out = []
        for ids, f, (lp, am, _) in zip(seqs, froms, self.backbone.score(seqs, froms)):
            out.append(dict(logprobs=lp, score=sequence_score(lp), top1_agreement=float(np.mean(am == np.asarray(ids[f:], dtype=np.int32)))))
        return out

    def _codes_to_ids(self, codes: Sequence[int]) -> List[int]:
        """The inverse of `_ids_to_codes`: code N -> the id of `<|speech_N|>`."""
        if self._speech_base is not None:
            return [int(self._speech_base) + int(c) for c in codes]
        return list(self.tokenizer.encode("".join(f"<|speech_{int(c)}|>" for c in codes), add_special_tokens=False))

    def encode_reference(self, ref_audio_path: str | Path):
        """ref:neutts/neutts.py:266-271: 16 kHz mono -> `codec.encode_code` -> 1-D int codes at 50 Hz.  On the encoder engine
        (kernels/enc.h) when encoder weights are loaded; one-off per speaker, off the synthesis hot path."""
        import torch
        wav = load_audio_16k(ref_audio_path)
        wav_tensor = torch.from_numpy(wav).float().unsqueeze(0).unsqueeze(0)  # [1, 1, T]
        with torch.no_grad():
            ref_codes = self.codec.encode_code(audio_or_path=wav_tensor).squeeze(0).squeeze(0)
        return ref_codes

    # ------------------------------------------------------------------------------------------ id-level hot path
    def _resolve_sampling(self, n: int, temperature=None, top_k=None, top_p=None, min_p=None, repetition: Optional[dict] = None) -> List[tuple]:
        """Per-call sampling overrides -> one checked (top_k, temperature, top_p, min_p, repetition_penalty, repetition_ignore_prompt) per
        utterance.  None = the instance attribute; a list / tuple / array gives one value per utterance (the batch entry points).  `repetition`:
        the entry point's remaining keywords, repetition_penalty / repetition_ignore_prompt.  ValueError on a bad value, before the engine is touched."""
        repetition = dict(repetition or {})
        rp, rip = repetition.pop("repetition_penalty", None), repetition.pop("repetition_ignore_prompt", None)
        if repetition:
            raise TypeError(f"unexpected keyword argument {sorted(repetition)[0]!r}")
        cols = []
        for name, v in (("top_k", top_k), ("temperature", temperature), ("top_p", top_p), ("min_p", min_p), ("repetition_penalty", rp),
                        ("repetition_ignore_prompt", rip)):
            if v is None:
                v = getattr(self, name)
            if isinstance(v, (list, tuple, np.ndarray)):
                v = list(v)
                if len(v) != n:
                    raise ValueError(f"{name}: {len(v)} values for {n} utterances")
                v = [getattr(self, name) if x is None else x for x in v]
            else:
                v = [v] * n
            cols.append(v)
        out = list(zip(*cols)) if n else []
        for i, (k, t, tp, mp, pen, ign) in enumerate(out):
            _check_sampling(k, t, tp, mp, f"utterance {i}: " if n > 1 else "")
            _check_repetition(pen, ign, f"utterance {i}: " if n > 1 else "")
        return [(int(k), float(t), float(tp), float(mp), float(pen), bool(ign)) for k, t, tp, mp, pen, ign in out]

    def _request_seed(self, index: int) -> int:
        # one Philox key per request: (call counter, index within the call)
        return (self._seed * 0x9E3779B97F4A7C15 + index * 0xD1B54A32D192ED03 + 1) & 0xFFFFFFFFFFFFFFFF

    def _sampling(self, prompt_len: int, index: int = 0, samp: Optional[Sequence[tuple]] = None) -> _hip.Sampling:
        if self._eos_id is None:
            raise RuntimeError("eos token id unknown: supply 'eos_token_id' with in-memory weights")
        seed = self._request_seed(index)
        top_k, temperature, top_p, min_p, pen, ign = samp[index] if samp is not None else (
            self.top_k, self.temperature, self.top_p, self.min_p, self.repetition_penalty, self.repetition_ignore_prompt)
        return _hip.Sampling(max_length=self.max_context, min_new_tokens=self.min_new_tokens, eos_token_id=self._eos_id,
                             do_sample=self.do_sample, top_k=top_k, temperature=temperature, seed=seed, top_p=top_p, min_p=min_p,
                             repetition_penalty=pen, prompt_ignore_length=prompt_len if ign else 0)

    def generate_codes(self, prompts: Sequence[Sequence[int]], *, temperature=None, top_k=None, top_p=None, min_p=None, **repetition) -> List[List[int]]:
        """Batched equivalent of `_infer_torch` (ref:neutts/neutts.py:334-352): new token ids per prompt.  The sampling overrides take one
        value for the call or one per prompt.  return_logprobs=True: (ids, logprobs), one float32 array per prompt beside its ids (the model's own
        log-probability of each token over the whole processed logits row: include/neutts_hip.h); best_of=N: the best of N candidates per prompt."""
        best_of, want = self._pop_scoring(len(prompts), repetition, "return_logprobs")
        samp = self._resolve_sampling(len(prompts), temperature, top_k, top_p, min_p, repetition)
        ids, lps = self._generate_scored(prompts, samp, best_of, want)
        return (ids, lps) if want else ids

    def _pop_scoring(self, n: int, kw: dict, flag: str):
        """The scoring keywords of an entry point's catch-all, taken out ahead of _resolve_sampling: best_of (one value or one per utterance;
        None = the attribute) and the entry point's own flag.  -> ([best_of per utterance], flag).  ValueError on a bad value."""
        want = kw.pop(flag, False)
        if not isinstance(want, (bool, np.bool_)):
            raise ValueError(f"{flag} must be True or False (got {want!r})")
        v = kw.pop("best_of", None)
        if isinstance(v, (list, tuple, np.ndarray)):
            v = list(v)
            if len(v) != n:
                raise ValueError(f"best_of: {len(v)} values for {n} utterances")
            v = [self.best_of if x is None else x for x in v]
        else:
            v = [self.best_of if v is None else v] * n
        for i, b in enumerate(v):
            _check_best_of(b, self.do_sample, f"utterance {i}: " if n > 1 else "")
        return [int(b) for b in v], bool(want)

    def _backbone_engines(self):
        return list(self.gang.engines) if self.gang is not None else [self.backbone]

    def _generate_scored(self, prompts, samp, best_of: Sequence[int], want: bool):
        """_generate with candidates and scores: utterance i is submitted best_of[i] times in ONE generate call (request index i * N + j with N the
        call's largest best_of, so every candidate has a seed of its own; the copies share the prompt's KV pages through prefix sharing) and the
        candidate with at least one speech token and the highest mean log-probability wins, ties to the lowest j.  -> (ids, logprobs) of the
        winners; logprobs is None unless scores were needed."""
        if not want and all(b == 1 for b in best_of):
            return self._generate(prompts, samp), None
        engines = self._backbone_engines()
        turned_on = [e for e in engines if not e.logprobs]
        if any(e.free_slots() != e.max_batch for e in turned_on):
            raise RuntimeError("log-probabilities cannot be switched on while a suspended stream holds a decode slot: finish or close the stream, "
                               "or build the instance with logprobs=True")
        N = max(best_of) if len(best_of) else 1
        rows, index, cand_prompts, cand_samp = [], [], [], []
        for i, p in enumerate(prompts):
            for j in range(best_of[i]):
                rows.append(i)
                index.append(i * N + j)
                cand_prompts.append(p)
                cand_samp.append(samp[i])
        try:
            for e in turned_on:
                e.set_logprobs(True)
            ids, lps = self._generate(cand_prompts, cand_samp, index=index, return_logprobs=True)
        finally:
            for e in turned_on:
                if e.logprobs:
                    e.set_logprobs(False)
        out_ids, out_lps = [None] * len(prompts), [None] * len(prompts)
        best = [None] * len(prompts)
        for r, i in enumerate(rows):
            score = sequence_score(lps[r]) if (best_of[i] == 1 or len(self._ids_to_codes(ids[r])) > 0) else float("-inf")
            if best[i] is None or score > best[i]:
                best[i], out_ids[i], out_lps[i] = score, ids[r], lps[r]
        return out_ids, out_lps

    def _generate(self, prompts: Sequence[Sequence[int]], samp: Sequence[tuple], index: Optional[Sequence[int]] = None,
                  return_logprobs: bool = False) -> List[List[int]]:
        """index: the request index each prompt's seed is derived from (default: its position); samp is indexed by position either way."""
        self._seed += 1
        # utterances of one speaker start with the same tokens (chat header + reference-text phones, ref :307,:315-325):
        # the engine keeps one copy of those KV pages and computes only what differs
        sampling = [self._sampling(len(p), i, samp) for i, p in enumerate(prompts)]
        if index is not None:
            for sp, k in zip(sampling, index):
                sp.seed = self._request_seed(k)
        kw = dict(return_logprobs=True) if return_logprobs else {}
        # more utterances than decode slots: freed slots are refilled about a tenth of an engine's slots at a time (24 of 256) -- a prompt
        # pass over a handful of prompts costs 1.5-2 us per token against 0.84 for 32 and more, an idle slot a step each
        # (profiles/r05m_probe_prefill_size.txt); scheduling only, the ids do not depend on it
        eng_slots = self.backbone.max_batch
        slots = eng_slots * (len(self.gang.engines) if self.gang is not None else 1)
        min_admit = max(1, min(24, eng_slots // 10)) if len(prompts) > slots else 1
        if self.gang is not None and len(prompts) > 1:
            return self.gang.generate(prompts, sampling, share_prefix=True, min_admit=min_admit, **kw)
        return self.backbone.generate(prompts, sampling, share_prefix=len(prompts) > 1, min_admit=min_admit, **kw)

    def _ids_to_codes(self, ids: Sequence[int]) -> List[int]:
        """ref :349 (tokenizer.decode) + :276 (regex): keep `<|speech_N|>` tokens, N = id - id(<|speech_0|>)."""
        if self._speech_base is not None:
            n_codes = 65536
            return [i - self._speech_base for i in ids if self._speech_base <= i < self._speech_base + n_codes]
        text = self.tokenizer.decode(list(ids), add_special_tokens=False)
        return [int(n) for n in _SPEECH_RE.findall(text)]

    def _ids_to_codes_array(self, ids: np.ndarray) -> np.ndarray:
        """`_ids_to_codes` on an id array (the batched stream's per-burst hand-off): the range test of the regex, vectorised, when
        the speech-token base is known and `_ids_to_codes` has not been replaced on the instance."""
        if self._speech_base is not None and "_ids_to_codes" not in self.__dict__:
            x = np.asarray(ids, dtype=np.int64) - self._speech_base
            return x[(x >= 0) & (x < 65536)].astype(np.int32)
        return np.asarray(self._ids_to_codes(np.asarray(ids).tolist()), dtype=np.int32)

    def decode_codes(self, codes: Sequence[Sequence[int]], sample_rate=None, encoding=None, speed=None, loudness=_INSTANCE) -> List[np.ndarray]:
        """Codec codes -> waveforms in the instance's output format, at the instance's speed and loudness (sample_rate= / encoding= / speed= /
        loudness= override them for this call; speed and loudness one value or one per utterance, loudness=None = off); no watermark, as before."""
        out = self._resolve_output(sample_rate, encoding)
        speed = self._resolve_speed(speed, len(codes))
        loud = self._resolve_loudness(loudness, len(codes))
        if out is None and speed is None and loud is None:
            return self.codec.engine.decode(codes)
        fmt = {} if out is None else dict(sample_rate=out[0], encoding=out[1], filter_width=out[2])
        if loud is None:
            return self.codec.engine.decode(codes, speed=speed, **fmt)
        return self.codec.engine.decode(codes, speed=speed, **loud, **fmt)

    def _resolve_loudness(self, loudness, n: int):
        """Per-call loudness: not given = the instance attribute; None = off.  -> None when no utterance has the option on (the calls of an instance
        without the stage), else CodecEngine.decode's three keywords with one checked target (or None) per utterance.  ValueError on a bad value,
        before the engine is touched."""
        given = loudness is not _INSTANCE
        loudness = loudness if given else self.loudness
        if _hip.loudness_params(loudness, self.loudness_peak, self.loudness_max_gain, n, "" if given else "instance ") is None:
            return None
        vals = list(loudness) if isinstance(loudness, (list, tuple, np.ndarray)) else [loudness] * n
        return dict(loudness=[None if v is None else float(v) for v in vals], loudness_peak=self.loudness_peak,
                    loudness_max_gain=self.loudness_max_gain)

    def _refuse_stream_loudness(self, loudness, who: str) -> None:
        if self._resolve_loudness(loudness, 1) is not None:
            what = f"loudness={loudness!r}" if loudness is not _INSTANCE else f"loudness={self.loudness!r} on the instance"
            raise ValueError(f"{who} has no loudness normalisation (got {what}): the gain of an utterance is known only at its end, after every chunk "
                             "but the last has left; loudness is a one-shot stage behind infer / infer_batch / decode_codes")

    def _resolve_speed(self, speed, n: int):
        """Per-call speed: None = the instance attribute.  -> None when every utterance runs at 1.0 (the calls of an instance without the stage), else
        one checked value per utterance.  ValueError on a bad value, before the engine is touched."""
        given = speed is not None
        speed = self.speed if speed is None else speed
        if _hip.speed_permille(speed, n, "" if given else "instance ") is None:
            return None
        return [float(v) for v in speed] if isinstance(speed, (list, tuple, np.ndarray)) else [float(speed)] * n

    def _refuse_stream_speed(self, speed, who: str) -> None:
        if self._resolve_speed(speed, 1) is not None:
            what = f"speed={speed!r}" if speed is not None else f"speed={self.speed!r} on the instance"
            raise ValueError(f"{who} speaks at speed 1.0 only (got {what}): the time stretch is a one-shot stage behind infer / infer_batch / "
                             "decode_codes; a stream's own speed is set by stream_speed=, which keeps the stretch's history on the device")

    def _resolve_stream_speed(self, speed, n: int):
        """Per-call speed of the stream entry points: None = the instance's stream_speed.  -> None when every utterance runs at 1.0 (the calls of an
        instance without the stage), else one checked value per utterance.  ValueError on a bad value, before a generator exists."""
        given = speed is not None
        speed = self.stream_speed if speed is None else speed
        if _hip.speed_permille(speed, n, "stream_" if given else "instance stream_") is None:
            return None
        return [float(v) for v in speed] if isinstance(speed, (list, tuple, np.ndarray)) else [float(speed)] * n

    def _resolve_output(self, sample_rate=None, encoding=None):
        """Per-call output format: None = the instance attribute.  -> None for the native format (24 kHz float32: the calls of an instance without
        the output stage), else the checked (sample_rate, encoding, filter_width).  ValueError on a bad value, before the engine is touched."""
        rate = self.output_sample_rate if sample_rate is None else sample_rate
        enc = self.output_encoding if encoding is None else encoding
        _check_output(rate, enc, self.output_filter_width, "" if sample_rate is not None or encoding is not None else "output_")
        return None if (int(rate) == self.sample_rate and enc == "f32") else (int(rate), enc, int(self.output_filter_width))

    def _refuse_stream_output(self, sample_rate, encoding, who: str) -> None:
        out = self._resolve_output(sample_rate, encoding)
        if out is not None:
            if out[0] != self.sample_rate:
                what = f"sample_rate={out[0]!r}" if sample_rate is not None else f"output_sample_rate={out[0]!r}"
            else:
                what = f"encoding={out[1]!r}" if encoding is not None else f"output_encoding={out[1]!r}"
            raise ValueError(f"{who} yields 24 kHz float32 chunks only (got {what}): resampling a stream needs filter history across chunk "
                             "edges; use infer / infer_batch for another output format, or convert the finished stream.  The chunks' own "
                             "format is set by stream_sample_rate= / stream_encoding= / stream_filter_width=, which keep that history on the device")

    def _resolve_stream_output(self, sample_rate=None, encoding=None, filter_width=None):
        """Per-call chunk format of the stream entry points: None = the instance's stream_* attribute (stream_filter_width None = output_filter_width).
        -> None for 24 kHz float32 (the calls of an instance without the stage), else the checked (sample_rate, encoding, filter_width)."""
        rate = self.stream_sample_rate if sample_rate is None else sample_rate
        enc = self.stream_encoding if encoding is None else encoding
        width = filter_width if filter_width is not None else (self.stream_filter_width if self.stream_filter_width is not None else self.output_filter_width)
        _check_output(rate, enc, width, "stream_")
        return None if (int(rate) == self.sample_rate and enc == "f32") else (int(rate), enc, int(width))

    @staticmethod
    def _format_chunks(conv, blended):
        """[(utterance, 24 kHz float32 chunk, last)] in order -> [(utterance, formatted chunk)]: one WavStream push per run of distinct utterances
        (a regular and a final window of one utterance in the same round are two chunks of its signal, in that order)."""
        out = []
        k0 = 0
        while k0 < len(blended):
            k1, seen = k0, set()
            while k1 < len(blended) and blended[k1][0] not in seen:
                seen.add(blended[k1][0])
                k1 += 1
            run = blended[k0:k1]
            outs = conv.push([b[1] for b in run], [b[0] for b in run], [b[2] for b in run])
            out += [(b[0], np.array(o)) for b, o in zip(run, outs)]
            k0 = k1
        return out

    def _stream_converter(self, n: int, fmt, spd=None):
        """The stages behind the cross-fade for the host loops' blended chunks: the chunked output stage (a WavStream of n rows), or with speeds the
        chunked time stretch with that stage behind it (a SpeedStream); None when there is neither.  The longest chunk is a final window's frame."""
        if fmt is None and spd is None:
            return None
        longest = (self.streaming_frames_per_chunk + self.streaming_lookforward + 2 * self.streaming_overlap_frames) * self.hop_length
        if spd is None:
            return self.codec.engine.stream_converter(n, fmt[0], fmt[1], fmt[2], max_chunk_samples=longest)
        fmt = (None, "f32", None) if fmt is None else fmt
        return self.codec.engine.stream_stretcher(n, spd, fmt[0], fmt[1], fmt[2], max_chunk_samples=longest)

    def _decode_formatted(self, codes: Sequence[Sequence[int]], out, speed=None, loud=None) -> List[np.ndarray]:
        """One codec pass with the time stretch (speed: None, or one value per utterance), the loudness normalisation (loud: None, or
        _resolve_loudness's keywords) and the device output stage (out: None = native) behind it, in that order.
        A watermarker is a host library that works on the 24 kHz float waveform: with one present the order is decode with the speed and the loudness
        in the native format, watermark on the host, then the output stage alone (CodecEngine.convert)."""
        eng = self.codec.engine
        fmt = {} if out is None else dict(sample_rate=out[0], encoding=out[1], filter_width=out[2])
        loud = loud or {}
        if self.watermarker is None:
            return eng.decode(codes, speed=speed, **loud, **fmt)
        wavs = [self.watermarker.apply_watermark(w, sample_rate=24_000) for w in eng.decode(codes, speed=speed, **loud)]
        return wavs if out is None else eng.convert(wavs, **fmt)

    def _decode_ids(self, ids: Sequence[int]) -> np.ndarray:
        speech_ids = self._ids_to_codes(ids)
        if len(speech_ids) > 0:
            return self.codec.engine.decode([speech_ids])[0]
        raise ValueError("No valid speech tokens found in the output.")

    def _decode(self, codes: str) -> np.ndarray:
        """String form kept for callers of the reference's private helper (ref:neutts/neutts.py:273-295)."""
        speech_ids = [int(num) for num in _SPEECH_RE.findall(codes)]
        if len(speech_ids) > 0:
            return self.codec.engine.decode([speech_ids])[0]
        raise ValueError("No valid speech tokens found in the output.")

    # ------------------------------------------------------------------------------------------ text front-end
    def _to_phones(self, text: str) -> str:
        if self.phonemizer is None:
            try:
                from phonemizer.backend import EspeakBackend
            except ImportError as e:
                raise ImportError("Text input needs `phonemizer` + espeak-ng (ref:requirements.txt:4); id-level entry "
                                  "points (generate_codes / decode_codes) do not.") from e
            print("Loading phonemizer...")
            self.phonemizer = EspeakBackend(language="en-us", preserve_punctuation=True, with_stress=True)
        phones = self.phonemizer.phonemize([text])
        return " ".join(phones[0].split())

    def _apply_chat_template(self, ref_codes, ref_text: str, input_text: str) -> List[int]:
        """Prompt ids exactly as ref:neutts/neutts.py:303-332 builds them."""
        tk = self.tokenizer
        input_text = self._to_phones(ref_text) + " " + self._to_phones(input_text)
        speech_replace = tk.convert_tokens_to_ids("<|SPEECH_REPLACE|>")
        speech_gen_start = tk.convert_tokens_to_ids("<|SPEECH_GENERATION_START|>")
        text_replace = tk.convert_tokens_to_ids("<|TEXT_REPLACE|>")
        text_prompt_start = tk.convert_tokens_to_ids("<|TEXT_PROMPT_START|>")
        text_prompt_end = tk.convert_tokens_to_ids("<|TEXT_PROMPT_END|>")
        input_ids = tk.encode(input_text, add_special_tokens=False)
        chat = """user: Convert the text to speech:<|TEXT_REPLACE|>\nassistant:<|SPEECH_REPLACE|>"""
        ids = tk.encode(chat)
        i = ids.index(text_replace)
        ids = ids[:i] + [text_prompt_start] + input_ids + [text_prompt_end] + ids[i + 1:]
        j = ids.index(speech_replace)
        codes_str = "".join(f"<|speech_{c}|>" for c in _to_list(ref_codes))
        codes = tk.encode(codes_str, add_special_tokens=False)
        return ids[:j] + [speech_gen_start] + list(codes)

    # ------------------------------------------------------------------------------------------ streaming
    def _infer_stream_hip(self, prompt_ids: List[int], ref_codes: List[int], samp: Optional[Sequence[tuple]] = None,
                          fmt=_INSTANCE_FORMAT, spd=None) -> Generator[np.ndarray, None, None]:
        """Window / cross-fade semantics of ref:neutts/neutts.py:401-465 (Appendix C of SURVEY.md), token by token.
        The backbone and the codec are separate engines on separate HIP streams: the next `chunk` decode steps are
        enqueued (asynchronously) BEFORE the codec pass of the chunk that just became decodable, so the codec runs
        beside the backbone instead of between its bursts; the host only blocks in `read()`.  With a chunk format (`fmt`) every blended chunk
        goes through the chunked output stage (a WavStream of one row) behind the cross-fade, with a speed (`spd`: None or [speed]) through the chunked
        time stretch ahead of it (a SpeedStream); a watermarker still sees 24 kHz float32 windows at speed 1."""
        if fmt is _INSTANCE_FORMAT:
            fmt = self._resolve_stream_output()
        conv = self._stream_converter(1, fmt, spd)
        emit = (lambda x, last=False: x) if conv is None else (lambda x, last=False: conv.push([x], last=last)[0])
        eng = self.backbone
        self._seed += 1
        slot = eng.acquire_slot()         # from the engine's pool: a stream that is still open never shares its slot
        try:
            eng.prefill([prompt_ids], [slot], [self._sampling(len(prompt_ids), 0, samp)])
        except Exception:
            eng.release(slot)
            raise
        token_cache: List[int] = list(ref_codes)          # codec codes (the reference caches "<|speech_N|>" strings)
        n_decoded_tokens = len(ref_codes)
        n_seen = 0
        hop = self.hop_length
        stride = self.streaming_stride_samples
        chunk, look_f, look_b, ovl = (self.streaming_frames_per_chunk, self.streaming_lookforward,
                                      self.streaming_lookback, self.streaming_overlap_frames)

        blend = _StreamBlender(stride)

        try:
            finished = False
            while not finished:
                ids, finished = eng.read(slot)            # blocks until the steps enqueued so far are done
                if not finished and self.streaming_overlap_compute:
                    eng.decode(chunk)                     # async: runs while the codec below decodes the last chunk
                new = self._ids_to_codes(ids[n_seen:])
                n_seen = len(ids)
                for c in new:
                    token_cache.append(c)
                    if len(token_cache) - n_decoded_tokens >= chunk + look_f:
                        t0 = max(n_decoded_tokens - look_b - ovl, 0)
                        t1 = n_decoded_tokens + chunk + look_f + ovl
                        s0 = (n_decoded_tokens - t0) * hop
                        s1 = s0 + (chunk + 2 * ovl) * hop
                        recon = self.codec.engine.decode([token_cache[t0:t1]])[0]
                        if self.watermarker is not None:
                            recon = self.watermarker.apply_watermark(recon, sample_rate=24_000)
                        n_decoded_tokens += chunk
                        yield emit(blend.push(np.array(recon[s0:s1])))
                if not finished and not self.streaming_overlap_compute:
                    eng.decode(chunk)                     # serial variant (A/B aid): backbone waits for the codec
            remaining = len(token_cache) - n_decoded_tokens
            if remaining > 0:
                t0 = max(len(token_cache) - (look_b + ovl + remaining), 0)
                s0 = (len(token_cache) - t0 - remaining - ovl) * hop
                recon = self.codec.engine.decode([token_cache[t0:]])[0]
                if self.watermarker is not None:
                    recon = self.watermarker.apply_watermark(recon, sample_rate=24_000)
                yield emit(blend.push(np.array(recon[s0:]), last=True), last=True)
            elif conv is not None and blend.prev is not None:        # the tokens ended on a window's edge (lookforward 0 only): what the stage holds back
                yield emit(np.zeros(0, dtype=np.float32), last=True)
        finally:
            eng.sync()
            eng.release(slot)
            if conv is not None:
                conv.close()


    # ---- device-side streaming (csrc/stream.cpp, ABI 6)
    def _stream_on_device(self, ref_codes) -> bool:
        # the device path covers what the class does by default: ids -> codes by the speech-token range (or the synthetic benchmark's
        # modulo rule), no watermarker (Perth runs on the host, ref:neutts/neutts.py:422-425), every stream opened by >= overlap codes
        if self.watermarker is not None or not getattr(self, "stream_on_device", True):
            return False
        if not getattr(self, "_stream_modulo", 0) and (self._speech_base is None or "_ids_to_codes" in self.__dict__):
            return False
        if self.streaming_lookforward < 2 * self.streaming_overlap_frames or 2 * self.streaming_overlap_frames >= self.streaming_frames_per_chunk:
            return False                   # (ntts_streams_create refuses these; the host loop slices like the reference does)
        return min(len(rc) for rc in ref_codes) >= self.streaming_overlap_frames

    def _stream_batch_device(self, slots, ref_codes, fmt=None, spd=None):
        """The loop of _infer_stream_batch_hip with the token caches, the window assembly, the 27-frame slice and the cross-fade on the
        device (ntts_streams_*): per burst the host waits for a snapshot of 2 n integers, enqueues the next burst, and receives each
        stream's new samples.  Same windows, same arithmetic (kernels/stream.h restates numpy's operations one by one): the chunks are
        bit-identical to the host path's."""
        eng = self.backbone
        chunk, look_f = self.streaming_frames_per_chunk, self.streaming_lookforward
        mod = int(getattr(self, "_stream_modulo", 0))
        ss = _hip.StreamSet(eng, self.codec.engine, slots, ref_codes, int(eng.cfg["max_context"]), chunk, look_f, self.streaming_lookback,
                            self.streaming_overlap_frames, self.hop_length, 0 if mod else int(self._speech_base), mod or 65536, bool(mod), fmt=fmt,
                            speed=spd)
        try:
            # the first window is complete once chunk + lookforward tokens exist (ref :401-404) and the prompt pass produced one of them
            steps = chunk + look_f - 1
            while True:
                ss.pump_begin()                           # behind everything enqueued so far
                running = ss.pump_wait()
                if running and self.streaming_overlap_compute:
                    eng.decode(steps)                     # async: runs beside the codec passes of pump_end
                more = True
                while more:
                    chunks, _, more = ss.pump_end()
                    for i, samples, _last in chunks:
                        yield i, np.array(samples)        # (the pinned buffer is reused by the next pump)
                if running and not self.streaming_overlap_compute:
                    eng.decode(steps)
                if not running:
                    break
                steps = chunk
        finally:
            ss.close()

    def _gang_codec_engines(self):
        """One codec engine per engine of the gang, each on that engine's lane stream (engine k's codec passes in engine k's hardware
        queue: four queues, four lanes -- _hip.EngineGang); the first one is the class's own."""
        if self._gang_codecs is None:
            cfg, sd, dev = self._codec_spec
            engs = [self.codec.engine]
            for _ in self.gang.engines[1:]:
                c = _hip.CodecEngine(cfg, dev, self._lib_path)
                c.load_state_dict(sd)
                engs.append(c)
            for k, c in enumerate(engs):
                if self.gang.lane(k):
                    c.set_stream(self.gang.lane(k))
            self._gang_codecs = engs
            self._gang_codec0_lent = True
        elif not getattr(self, "_gang_codec0_lent", False) and self.gang.lane(0):
            self._gang_codecs[0].set_stream(self.gang.lane(0))     # (handed back at the end of the previous gang call)
            self._gang_codec0_lent = True
        return self._gang_codecs

    def _infer_stream_batch_gang(self, prompts: List[List[int]], ref_codes: List[List[int]], samp: Optional[Sequence[tuple]] = None, fmt=None,
                                 spd=None):
        """infer_stream_batch over an ENGINE GANG (BASELINE configs[4]'s literal shape: ref:neutts/neutts.py:373-465
        for many utterances at once).  The utterances are dealt out in admission groups over the gang's engines; every group is a
        device-side stream set (ntts_streams_*) on its engine, the engine's codec engine on the same lane.  Per turn of an engine:
        [snapshot + windows of its sets -> codec pass -> chunks out] [admit its next group: prompt pass] [next decode burst] -- the other
        engines' bursts run meanwhile.  Opt-in (`stream_on_gang = True`: it pays for the fp8 Nano-sized model, not for NeuTTS-Air bf16, see
        _infer_stream_batch_hip).  Group size `stream_admit`: by default ONE group per engine (the streams split evenly, at least 64
        per engine), all prompt passes at once and the chains side by side from then on -- 512 streams of the fp8 Nano-sized model over
        four 128-slot engines: 150.2 k codec-tokens/s, first audio 152 / 168 / 186 ms (first / median / last stream) against 144.2 k and
        182 ms on one 512-slot engine; smaller groups stagger the admissions (a group's first audio waits for ITS prompt pass only) but a
        decode chain next to another engine's prompt pass crawls: groups of 64 144.1 k, 157 / 177 / 203 ms; of 32 125.3 k
        (profiles/r05o_sweep_stream_gang.txt).  A window is defined by token COUNTS (30 undecoded tokens, csrc/stream.cpp pump_end), not
        by when it is looked for: the chunks are those of the single stream, bit for bit, whatever the burst boundaries."""
        gang = self.gang
        G = len(gang.engines)
        codecs = self._gang_codec_engines()
        n = len(prompts)
        self._seed += 1
        admit = getattr(self, "stream_admit", None)
        if not admit:
            groups = min(G, max(1, n // 64))
            admit = (n + groups - 1) // groups
        admit = max(1, int(admit))
        chunk, look_f = self.streaming_frames_per_chunk, self.streaming_lookforward
        mod = int(getattr(self, "_stream_modulo", 0))
        room = [e.free_slots() for e in gang.engines]
        if n > sum(room):
            raise ValueError(f"{n} utterances exceed the gang's free decode slots ({sum(room)})")
        # groups of at most `admit` streams, each to the engine with the most room left (ties: round-robin), a group no larger than that room
        pending: List[List[List[int]]] = [[] for _ in range(G)]
        i0, turn = 0, 0
        while i0 < n:
            k = max(range(G), key=lambda j: (room[j], -((j - turn) % G)))
            m = min(admit, room[k], n - i0)
            pending[k].append(list(range(i0, i0 + m)))
            room[k] -= m
            i0 += m
            turn += 1
        active: List[list] = [[] for _ in range(G)]           # per engine: [stream set, utterance indices, slots]
        try:
            while any(pending) or any(active):
                for k, eng in enumerate(gang.engines):
                    if not pending[k] and not active[k]:
                        continue
                    running = 0
                    for item in active[k]:
                        item[0].pump_begin()                  # behind the burst enqueued in this engine's previous turn
                    for item in active[k]:
                        running += item[0].pump_wait()
                    for item in list(active[k]):
                        ss, idx, slots = item[0], item[1], item[2]
                        more = True
                        while more:
                            chunks, _, more = ss.pump_end()   # codec pass + cross-fade on the engine's lane, ahead of its next burst
                            for i, samples, _last in chunks:
                                yield idx[i], np.array(samples)
                        if ss.done() == ss.n:
                            ss.close()
                            eng.release_many(slots)
                            item[2] = []
                            active[k].remove(item)
                    admitted = False
                    if pending[k]:
                        idx = pending[k].pop(0)
                        slots = [eng.acquire_slot() for _ in idx]
                        item = [None, idx, slots]
                        active[k].append(item)                # (registered first: its slots are released on any exit path)
                        budget = eng.cfg.get("max_prefill_tokens", 0) or 16384
                        i0 = 0
                        while i0 < len(idx):
                            i1, used = i0, 0
                            while i1 < len(idx) and (i1 == i0 or used + len(prompts[idx[i1]]) <= budget):
                                used += len(prompts[idx[i1]])
                                i1 += 1
                            eng.prefill([prompts[i] for i in idx[i0:i1]], slots[i0:i1], [self._sampling(len(prompts[i]), i, samp) for i in idx[i0:i1]])
                            i0 = i1
                        item[0] = _hip.StreamSet(eng, codecs[k], slots, [ref_codes[i] for i in idx], int(eng.cfg["max_context"]), chunk, look_f,
                                                 self.streaming_lookback, self.streaming_overlap_frames, self.hop_length,
                                                 0 if mod else int(self._speech_base), mod or 65536, bool(mod), fmt=fmt,
                                                 speed=None if spd is None else [spd[i] for i in idx])
                        admitted = True
                        running += len(idx)
                    if running:
                        # a new group holds one token per stream: lookforward - 1 steps now and whole chunks from then on complete its
                        # first window (chunk + lookforward tokens) exactly at a burst boundary; the older groups just run ahead.
                        # (Measured and not kept: bursts sized to whatever the set nearest to its next window needs -- more, shorter
                        #  bursts and pump rounds: 127.0 k instead of 143.5 k codec-tokens/s at 512 streams, first audio 182 instead of
                        #  157 ms; profiles/r05g_bench_nano-fp8_stream_*.json)
                        eng.decode(look_f - 1 if (admitted and look_f > 1) else chunk)
        finally:
            try:
                codecs[0].set_stream(None)               # the class's own codec engine goes back to its stream for the non-gang calls that follow
            except _hip.NeuTTSHipError:                  # (infer, infer_stream, infer_stream_batch on engine 0); re-lent by the next gang call
                pass
            self._gang_codec0_lent = False
            for k, eng in enumerate(gang.engines):
                for item in active[k]:
                    if item[0] is not None:
                        item[0].close()
                if any(item[2] for item in active[k]):
                    try:
                        eng.sync()
                    except _hip.NeuTTSHipError:
                        pass
                    for item in active[k]:
                        for sl in item[2]:
                            try:
                                eng.release(sl)
                            except _hip.NeuTTSHipError:
                                pass

    def _infer_stream_batch_hip(self, prompts: List[List[int]], ref_codes: List[List[int]], samp: Optional[Sequence[tuple]] = None,
                                fmt=_INSTANCE_FORMAT, spd=None):
        # fmt: the chunks' format -- None = 24 kHz float32, (sample_rate, encoding, filter_width), or (the default) the instance's stream_* attributes
        # spd: the chunks' speeds -- None = all at 1.0, or one value per utterance
        if fmt is _INSTANCE_FORMAT:
            fmt = self._resolve_stream_output()
        # (stream_on_gang: off unless the caller sets it -- it pays for one of the two models measured.  512 streams of the fp8 Nano-sized model
        #  over four 128-slot engines, one admission group per engine: 150.2 k codec-tokens/s and first audio 152 / 168 / 186 ms against 144.2 k /
        #  182 ms on ONE 512-slot engine; NeuTTS-Air bf16: 256 streams over 4 x 64 slots 80.3 k against 100.5 k on one engine, 512 streams over
        #  4 x 128 111.9 k against 114.9 k -- four chains stream Air's larger weights four times; profiles/r05o_sweep_stream_gang*.txt)
        if (self.gang is not None and len(prompts) > 1 and getattr(self, "stream_on_gang", False) and self._stream_on_device(ref_codes)):
            yield from self._infer_stream_batch_gang(prompts, ref_codes, samp, fmt, spd)
            return
        eng = self.backbone
        n = len(prompts)
        self._seed += 1
        if eng.free_slots() < n:
            raise ValueError(f"{n} utterances exceed the engine's {eng.free_slots()} free decode slots")
        slots = [eng.acquire_slot() for _ in range(n)]
        budget = eng.cfg.get("max_prefill_tokens", 0) or 16384       # the prefill workspace bounds one call
        try:
            i0 = 0
            while i0 < n:
                i1, used = i0, 0
                while i1 < n and (i1 == i0 or used + len(prompts[i1]) <= budget):
                    used += len(prompts[i1])
                    i1 += 1
                eng.prefill(prompts[i0:i1], slots[i0:i1], [self._sampling(len(prompts[i]), i, samp) for i in range(i0, i1)])
                i0 = i1
        except Exception:                  # a later group failed: the earlier groups' slots must not stay RUNNING
            eng.sync()
            for s in slots:
                eng.release(s)
            raise
        hop, stride = self.hop_length, self.streaming_stride_samples
        chunk, look_f, look_b, ovl = (self.streaming_frames_per_chunk, self.streaming_lookforward,
                                      self.streaming_lookback, self.streaming_overlap_frames)
        if self._stream_on_device(ref_codes):
            try:
                yield from self._stream_batch_device(slots, ref_codes, fmt, spd)
            finally:
                eng.sync()
                for s in slots:
                    eng.release(s)
            return
        # ---- host path (a watermarker is a host library; an id -> code rule other than the speech-token range): per utterance the
        #      reference codes + generated codes in one int32 row (the reference caches "<|speech_N|>" strings)
        cap = max(len(rc) for rc in ref_codes) + int(eng.cfg["max_context"]) + 1
        cache = np.zeros((n, cap), dtype=np.int32)
        clen = np.zeros(n, dtype=np.int64)                # tokens in cache[i]
        for i, rc in enumerate(ref_codes):
            cache[i, :len(rc)] = rc
            clen[i] = len(rc)
        n_dec = clen.copy()                               # tokens already turned into audio
        n_seen = [0] * n
        blend = [_StreamBlender(stride) for _ in range(n)]
        done = [False] * n                                # final chunk emitted
        need = chunk + look_f                             # undecoded tokens that make a window decodable (ref :401-404)
        conv = None
        try:
            conv = self._stream_converter(n, fmt, spd)    # the stages behind the cross-fade (time stretch, output format): one row per utterance
            pm = _hip.speed_permille(spd, n)
            held = [fmt is not None or (pm is not None and pm[i] != 1000) for i in range(n)]        # utterances whose stage holds samples back
            while not all(done):
                ids_all, n_new_all, fin_all = eng.read_all_array()    # blocks until the bursts enqueued so far are done
                ids, n_new, fin = ids_all[slots], n_new_all[slots], fin_all[slots]     # row i = utterance i
                running = [i for i in range(n) if not done[i] and not fin[i]]
                if running and self.streaming_overlap_compute:
                    eng.decode(chunk)                     # async: runs beside the codec pass below
                jobs = []                                 # (utterance, window codes, s0, s1 or None, last)
                flush = []                                # formatted utterances that end without a final window
                for i in range(n):
                    if done[i]:
                        continue
                    if n_new[i] > n_seen[i]:
                        new = self._ids_to_codes_array(ids[i, n_seen[i]:n_new[i]])
                        cache[i, clen[i]:clen[i] + len(new)] = new
                        clen[i] += len(new)
                        n_seen[i] = int(n_new[i])
                    # The reference checks after EVERY appended token and slices `token_cache[start : n_dec + 31]` at the moment the
                    # 30th undecoded token arrives -- the slice then ends at n_dec + 30, whatever arrives later.  Same windows here
                    # without the per-token loop: as many as the tokens of this burst complete, each ending at its own n_dec + 30.
                    while clen[i] - n_dec[i] >= need:
                        t0 = max(int(n_dec[i]) - look_b - ovl, 0)
                        t1 = int(n_dec[i]) + need
                        s0 = (int(n_dec[i]) - t0) * hop
                        jobs.append((i, cache[i, t0:t1], s0, s0 + (chunk + 2 * ovl) * hop, False))
                        n_dec[i] += chunk
                    if fin[i]:
                        remaining = int(clen[i] - n_dec[i])
                        if remaining > 0:
                            t0 = max(int(clen[i]) - (look_b + ovl + remaining), 0)
                            s0 = (int(clen[i]) - t0 - remaining - ovl) * hop
                            jobs.append((i, cache[i, t0:clen[i]], s0, None, True))
                        elif conv is not None and held[i] and (blend[i].prev is not None or any(j[0] == i for j in jobs)):
                            flush.append(i)               # (the tokens ended on a window's edge: lookforward 0 only)
                        done[i] = True
                if jobs:
                    wavs = self.codec.engine.decode([j[1] for j in jobs], reuse_output=True)     # one batched codec pass; views of the
                    pieces = []                                                                   # engine's pinned buffer: EVERY job's slice is
                    for (i, _, s0, s1, last), recon in zip(jobs, wavs):                           # copied out before the first yield -- while the
                        if self.watermarker is not None:                                         # generator is suspended another decode on this
                            recon = self.watermarker.apply_watermark(recon, sample_rate=24_000)   # codec engine may overwrite that buffer
                        pieces.append((i, np.array(recon[s0:s1]), last))
                    del wavs
                    if conv is None:
                        for i, piece, last in pieces:
                            yield i, blend[i].push(piece, last=last)
                    else:                                  # blended on the host, then the chunked output stage
                        yield from self._format_chunks(conv, [(i, blend[i].push(piece, last=last), last) for i, piece, last in pieces])
                if flush:                                 # what the stage holds back of them: chunks of their own, behind the round's others
                    yield from self._format_chunks(conv, [(i, np.zeros(0, dtype=np.float32), True) for i in flush])
                if running and not self.streaming_overlap_compute:
                    eng.decode(chunk)
        finally:
            eng.sync()
            for s in slots:
                eng.release(s)
            if conv is not None:
                conv.close()


def _engine_config_from_hf(hc) -> Dict[str, object]:
    """AutoModelForCausalLM's dispatch (ref:neutts/neutts.py:164), restated for the decoder family the engine implements:
    the pre-norm RoPE / GQA / SwiGLU decoder of Qwen2 (NeuTTS-Air), Llama-style checkpoints (no q/k/v bias, possibly an
    untied head) and Qwen3 (per-head q/k RMSNorm, head_dim 128: the engine's general attention path, round 6).  Everything is read from config.json; what the kernels cannot do fails HERE with the reason, not later
    with wrong audio."""
    mt = getattr(hc, "model_type", "")
    if mt not in ("qwen2", "llama", "mistral", "qwen3"):
        raise NotImplementedError(f"backbone model_type {mt!r}: the MI355X engine implements the Qwen2 / Llama decoder "
                                  "family (NeuTTS-Air is 'qwen2')")
    head_dim = getattr(hc, "head_dim", None) or hc.hidden_size // hc.num_attention_heads
    if head_dim not in (64, 128):
        raise NotImplementedError(f"backbone head_dim {head_dim}: the attention kernels are built for head_dim 64 and 128")
    if getattr(hc, "sliding_window", None) and getattr(hc, "use_sliding_window", False):
        raise NotImplementedError("sliding-window attention is not implemented")
    if getattr(hc, "mlp_bias", False):
        raise NotImplementedError("MLP biases are not implemented")
    return dict(vocab_size=hc.vocab_size, hidden_size=hc.hidden_size, intermediate_size=hc.intermediate_size,
                num_layers=hc.num_hidden_layers, num_heads=hc.num_attention_heads,
                num_kv_heads=getattr(hc, "num_key_value_heads", None) or hc.num_attention_heads, rms_eps=hc.rms_norm_eps,
                head_dim=head_dim, tie_word_embeddings=bool(getattr(hc, "tie_word_embeddings", True)),
                attention_bias=bool(getattr(hc, "attention_bias", mt == "qwen2")),
                qk_norm=(mt == "qwen3"))       # Qwen3Attention: q_norm / k_norm (RMSNorm over head_dim) on every head before RoPE


def _to_list(codes) -> List[int]:
    if hasattr(codes, "tolist"):
        return [int(c) for c in np.asarray(codes.cpu() if hasattr(codes, "cpu") else codes).reshape(-1).tolist()]
    return [int(c) for c in codes]


def _safetensors_shards(repo) -> List[str]:
    """*.safetensors files of a checkpoint: a local directory, or a hub repo id resolved through the local HF cache /
    a download of exactly those files."""
    import glob
    import os
    repo = str(repo)
    if os.path.isdir(repo):
        return sorted(glob.glob(os.path.join(repo, "*.safetensors")))
    try:
        from huggingface_hub import snapshot_download
        d = snapshot_download(repo, allow_patterns=["*.safetensors", "*.json"])
        return sorted(glob.glob(os.path.join(d, "*.safetensors")))
    except Exception:
        return []


def _default_rope_theta(hc) -> Optional[float]:
    """rope_theta when the checkpoint uses the default RoPE parametrisation (what NeuTTS-Air / Qwen2.5 do), else None
    (the caller then lets transformers build the rotary embedding and reads its inv_freq buffer)."""
    rp = getattr(hc, "rope_parameters", None) or getattr(hc, "rope_scaling", None)
    if isinstance(rp, dict):
        if rp.get("rope_type", rp.get("type", "default")) != "default":
            return None
        if "rope_theta" in rp:
            return float(rp["rope_theta"])
    theta = getattr(hc, "rope_theta", None)
    return float(theta) if theta is not None else None


class _SafetensorsStateDict:
    """Minimal `.items()` view over safetensors shards: one tensor in host memory at a time."""

    def __init__(self, shards: Sequence[str]):
        self.shards = list(shards)

    def items(self):
        from safetensors import safe_open
        for path in self.shards:
            with safe_open(path, framework="pt", device="cpu") as f:
                for k in f.keys():
                    if not k.endswith("inv_freq"):
                        yield k, f.get_tensor(k)


def neucodec_to_xcodec2_names(sd: Dict[str, object], strict: bool = True) -> Dict[str, object]:
    """Original `neucodec` state-dict keys -> the xcodec2 parameter names the codec engine loads.
    Fused `att.c_attn.weight [3H, H]` rows are split q | k | v.

    The key layout is the survey's reading of the neucodec package, which cannot be installed offline, so this function
    does not trust it: with `strict` (the default) EVERY decoder-side tensor the engine needs must be found under its
    expected source key, and every decoder-side source key (`generator.backbone.*`, `generator.head.*`,
    `generator.quantizer.project_out.*`, `fc_post_a.*`) must be consumed -- otherwise a ValueError lists the missing and
    the unrecognised keys, instead of a late 'tensor X not loaded' from the engine or, worse, silently skipped weights."""
    out: Dict[str, object] = {}
    missing: List[str] = []
    used = set()

    def put(dst, src):
        if src in sd:
            out[dst] = sd[src]
            used.add(src)
        else:
            missing.append(f"{src} (-> {dst})")

    put("quantizer.project_out.weight", "generator.quantizer.project_out.weight")
    put("quantizer.project_out.bias", "generator.quantizer.project_out.bias")
    put("decoder.fc.weight", "fc_post_a.weight")
    put("decoder.fc.bias", "fc_post_a.bias")
    put("decoder.embed.weight", "generator.backbone.embed.weight")
    put("decoder.embed.bias", "generator.backbone.embed.bias")
    for net in ("prior_net", "post_net"):
        for b in range(2):
            for part in ("norm1", "conv1", "norm2", "conv2"):
                for wb in ("weight", "bias"):
                    put(f"decoder.{net}.{b}.{part}.{wb}", f"generator.backbone.{net}.{b}.{part}.{wb}")
    i = 0
    while f"generator.backbone.transformers.{i}.att.c_attn.weight" in sd:
        p, q = f"generator.backbone.transformers.{i}.", f"decoder.layers.{i}."
        w = sd[p + "att.c_attn.weight"]
        used.add(p + "att.c_attn.weight")
        if w.shape[0] % 3:
            raise ValueError(f"{p}att.c_attn.weight: {tuple(w.shape)} is not a fused q|k|v matrix")
        h = w.shape[0] // 3
        out[q + "self_attn.q_proj.weight"], out[q + "self_attn.k_proj.weight"], out[q + "self_attn.v_proj.weight"] = (
            w[:h], w[h:2 * h], w[2 * h:])
        put(q + "self_attn.o_proj.weight", p + "att.c_proj.weight")
        put(q + "input_layernorm.weight", p + "att_norm.weight")
        put(q + "post_attention_layernorm.weight", p + "ffn_norm.weight")
        put(q + "mlp.fc1.weight", p + "mlp.fc1.weight")
        put(q + "mlp.fc2.weight", p + "mlp.fc2.weight")
        i += 1
    if i == 0:
        missing.append("generator.backbone.transformers.0.att.c_attn.weight (-> decoder.layers.0.self_attn.{q,k,v}_proj.weight)")
    put("decoder.norm.weight", "generator.backbone.final_layer_norm.weight")
    put("decoder.norm.bias", "generator.backbone.final_layer_norm.bias")
    put("decoder.head.linear.weight", "generator.head.out.weight")
    put("decoder.head.linear.bias", "generator.head.out.bias")
    if not out:
        raise ValueError("no NeuCodec decoder tensors found in the state dict")
    # decoder-side source keys nobody asked for: buffers that carry no parameters are fine, anything else is a layout
    # this mapping does not know
    benign = ("generator.head.istft.window", "rotary", "inv_freq", "freqs_cis", "num_batches_tracked", "codebook",
              "implicit_codebook", "_levels", "_basis", "scales", "project_in")
    decoder_side = ("generator.backbone.", "generator.head.", "generator.quantizer.project_out", "fc_post_a.")
    unknown = sorted(k for k in sd if k.startswith(decoder_side) and k not in used and not any(b in k for b in benign))
    if strict and (missing or unknown):
        raise ValueError(
            "NeuCodec checkpoint does not match the expected decoder layout (SURVEY.md B.4):\n"
            + (f"  missing source keys ({len(missing)}): " + ", ".join(missing[:12]) + (" ..." if len(missing) > 12 else "") + "\n"
               if missing else "")
            + (f"  unrecognised decoder-side keys ({len(unknown)}): " + ", ".join(unknown[:12]) + (" ..." if len(unknown) > 12 else "")
               if unknown else ""))
    return out


def neucodec_encoder_to_xcodec2_names(sd: Dict[str, object], n_layers: int = 16) -> Dict[str, object]:
    """Original `neucodec` ENCODER-side state-dict keys -> the xcodec2 parameter names the encoder engine loads.

    Like the decoder mapping above, the key layout is a reading of the neucodec / xcodec2 sources that cannot be checked
    offline, so nothing is trusted: the w2v-BERT, adapter, fc and project_in tensors are looked up by name and every one
    must exist; the acoustic encoder (`CodecEnc.*`, weight-normalised convolutions + SnakeBeta activations inside nested
    nn.Sequential containers) is mapped by MODULE ORDER and checked by SHAPE -- 1 input conv, per ratio 3 x (snake, conv 7,
    snake, conv 1) + snake + strided conv, then snake + conv 3 -- with weight norm folded (w = g * v / ||v||).  Any mismatch
    raises ValueError that lists the keys (there is no other encoder to fall back to)."""
    import torch
    out: Dict[str, object] = {}
    missing: List[str] = []

    def put(dst, src):
        if src in sd:
            out[dst] = sd[src]
        else:
            missing.append(f"{src} (-> {dst})")

    for k in sd:
        if k.startswith("semantic_model.") and "masked_spec_embed" not in k:
            parts = k.split(".")
            if parts[1:3] == ["encoder", "layers"] and int(parts[3]) >= n_layers:
                continue                                   # neucodec reads hidden_states[16]: layers 17..24 never run
            if parts[1] in ("feature_projection", "encoder"):
                out["semantic_encoder." + k[len("semantic_model."):]] = sd[k]
    if not any(k.startswith("semantic_encoder.encoder.layers.") for k in out):
        missing.append("semantic_model.encoder.layers.* (w2v-BERT 2.0)")
    put("semantic_adapter.conv1.weight", "SemanticEncoder_module.initial_conv.weight")
    put("semantic_adapter.conv2.weight", "SemanticEncoder_module.residual_blocks.1.weight")
    put("semantic_adapter.conv2.bias", "SemanticEncoder_module.residual_blocks.1.bias")
    put("semantic_adapter.conv3.weight", "SemanticEncoder_module.residual_blocks.3.weight")
    put("semantic_adapter.conv3.bias", "SemanticEncoder_module.residual_blocks.3.bias")
    put("semantic_adapter.conv4.weight", "SemanticEncoder_module.final_conv.weight")
    put("fc_encoder.weight", "fc_prior.weight")
    put("fc_encoder.bias", "fc_prior.bias")
    put("quantizer.project_in.weight", "generator.quantizer.project_in.weight")
    put("quantizer.project_in.bias", "generator.quantizer.project_in.bias")
    # acoustic encoder: modules in registration order
    mods: Dict[str, Dict[str, object]] = {}
    for k, v in sd.items():
        if not k.startswith("CodecEnc.") or "filter" in k:
            continue
        for suf in ("parametrizations.weight.original0", "parametrizations.weight.original1", "weight_g", "weight_v", "weight",
                    "bias", "alpha", "beta"):
            if k.endswith("." + suf):
                mods.setdefault(k[: -len(suf) - 1], {})[suf] = v
                break
        else:
            missing.append(f"{k} (unrecognised acoustic-encoder tensor)")
    convs, snakes = [], []
    for name, t in mods.items():
        if "alpha" in t and "beta" in t:
            snakes.append((name, t["alpha"].reshape(-1), t["beta"].reshape(-1)))
            continue
        g = t.get("weight_g", t.get("parametrizations.weight.original0"))
        v = t.get("weight_v", t.get("parametrizations.weight.original1"))
        if g is not None and v is not None:
            w = v * (g.reshape(-1, 1, 1) / torch.linalg.vector_norm(v.float(), dim=(1, 2), keepdim=True).to(v.dtype))
        elif "weight" in t:
            w = t["weight"]
        else:
            missing.append(f"{name} (neither a convolution nor a SnakeBeta)")
            continue
        convs.append((name, w, t.get("bias")))
    n_ratios = (len(convs) - 2) // 7
    if missing or len(convs) != 2 + 7 * n_ratios or len(snakes) != 1 + 7 * n_ratios or n_ratios < 1:
        raise ValueError("NeuCodec checkpoint does not match the expected ENCODER layout: "
                         + (", ".join(missing[:12]) + (" ..." if len(missing) > 12 else "") if missing
                            else f"{len(convs)} convolutions / {len(snakes)} SnakeBeta activations under CodecEnc.*"))
    ci, si = iter(convs), iter(snakes)

    def conv(dst, k=None, cin=None):
        name, w, b = next(ci)
        if w.dim() != 3 or (k is not None and w.shape[2] != k) or (cin is not None and w.shape[1] != cin) or b is None:
            raise ValueError(f"acoustic encoder: {name} {tuple(w.shape)} is not the convolution expected at {dst}")
        out[dst + ".weight"], out[dst + ".bias"] = w, b
        return w.shape[0]

    def snake(dst, c):
        name, a, b = next(si)
        if a.numel() != c or b.numel() != c:
            raise ValueError(f"acoustic encoder: {name} has {a.numel()} channels, {c} expected at {dst}")
        out[dst + ".act.alpha"], out[dst + ".act.beta"] = a, b

    ch = conv("acoustic_encoder.conv1", 7, 1)
    for bi in range(n_ratios):
        b = f"acoustic_encoder.block.{bi}."
        for u in (1, 2, 3):
            snake(f"{b}res_unit{u}.snake1", ch)
            conv(f"{b}res_unit{u}.conv1", 7, ch)
            snake(f"{b}res_unit{u}.snake2", ch)
            conv(f"{b}res_unit{u}.conv2", 1, ch)
        snake(b + "snake1", ch)
        ch = conv(b + "conv1", None, ch)
    snake("acoustic_encoder.snake1", ch)
    conv("acoustic_encoder.conv2", 3, ch)
    return out

