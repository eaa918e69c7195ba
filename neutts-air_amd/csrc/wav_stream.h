// wav_stream.h -- the chunked output stage (kernels/codec.h wav_stream_kernel) as codec.cpp offers it to the two callers that launch it:
// ntts_wav_stream_* (codec.cpp: the stage alone on host chunks) and ntts_streams_pump_end_fmt (stream.cpp: behind the cross-fade).  Internal: not
// part of include/neutts_hip.h.  Errors go to the codec engine's message (ntts_codec_last_error).
#pragma once
#include <ntts/dev.h>

#include <stddef.h>
#include <stdint.h>

#include "../../include/neutts_hip.h"

namespace ntts {

struct WavStreamCore;      // per-stream counts and history of `n_streams` streams in one format, and room for `max_jobs` jobs per launch

int wav_core_create(ntts_codec* c, const ntts_wav_format* fmt, int n_streams, int max_chunk_samples, int max_jobs, WavStreamCore** out);
void wav_core_destroy(WavStreamCore* k);
bool wav_core_plain(const WavStreamCore* k);          // 24 kHz float32: nothing to compute
size_t wav_core_esz(const WavStreamCore* k);           // bytes per output element
long wav_core_out_stride(const WavStreamCore* k);      // elements per job row of the output buffer: the most a chunk of max_chunk_samples can emit
void* wav_core_out(const WavStreamCore* k);            // DEVICE [max_jobs][out_stride] elements
// output samples stream `u` emits for a chunk of n_new more samples, without touching its state
int64_t wav_core_peek(const WavStreamCore* k, int u, int n_new, bool last);
// job `job` of the coming launch: stream u takes n_new samples (its final chunk if `last`) in launch `phase` (0, or 1 for a stream's second job of
// the round); advances the stream's counts and returns the samples the job will write
int64_t wav_core_plan(WavStreamCore* k, int job, int u, int n_new, bool last, int phase);
// uploads jobs [0, n_jobs) and launches them on `st`: job j reads its n_new samples at in_dev + j * in_stride and writes row j of wav_core_out
int wav_core_run(WavStreamCore* k, int n_jobs, const float* in_dev, long in_stride, hipStream_t st);
// host arithmetic of ntts_wav_stream_count
int wav_stream_count_of(ntts_codec* c, const ntts_wav_format* fmt, int64_t n_in_total, bool last, int64_t* n_out_total);

// ---- the chunked time stretch (kernels/codec.h wav_stretch_stream_kernel) in the same shape, for the same two callers: ntts_speed_stream_* (codec.cpp)
// and ntts_streams_set_speed (stream.cpp: behind the cross-fade, ahead of the output stage).  A stream's speed is fixed with the first chunk of a
// signal and free again after its last.  The host holds counts only; positions, history and the state records stay on the device.
struct SpeedStreamCore;    // `n_streams` streams, rows for chunks of `max_chunk_samples` at speeds down to `pm_min`, room for `max_jobs` jobs per launch

int speed_core_create(ntts_codec* c, int n_streams, int max_chunk_samples, int pm_min, int max_jobs, SpeedStreamCore** out);
void speed_core_destroy(SpeedStreamCore* k);
long speed_core_out_stride(const SpeedStreamCore* k);  // floats per job row: the most a chunk of max_chunk_samples can emit at pm_min
long speed_core_pos_stride(const SpeedStreamCore* k);  // frames per job row of the positions
float* speed_core_out(const SpeedStreamCore* k);       // DEVICE [max_jobs][out_stride] 24 kHz float32
int* speed_core_pos(const SpeedStreamCore* k);         // DEVICE [max_jobs][pos_stride]: the positions each job decided (speeds other than 1000)
int speed_core_pm(const SpeedStreamCore* k, int u);    // the speed stream u's current signal began with; 0 between signals
int64_t speed_core_total(const SpeedStreamCore* k, int u);   // input samples of its current signal so far
// stretched samples stream `u` emits for a chunk of n_new more samples at pm, without touching its state
int64_t speed_core_peek(const SpeedStreamCore* k, int u, int pm, int n_new, bool last);
// job `job` of the coming launch (as wav_core_plan); *k0 / *k1 (may be null): the frames it decides
int64_t speed_core_plan(SpeedStreamCore* k, int job, int u, int pm, int n_new, bool last, int phase, int* k0, int* k1);
// uploads jobs [0, n_jobs) and launches them on `st`: job j reads its n_new samples at in_dev + j * in_stride and writes row j of speed_core_out
int speed_core_run(SpeedStreamCore* k, int n_jobs, const float* in_dev, long in_stride, hipStream_t st);
// host arithmetic of ntts_speed_stream_count (pm checked by the caller)
int64_t speed_stream_count_of(int pm, int64_t n_in_total, bool last);
int64_t speed_chunk_out_max(int64_t max_chunk_samples, int pm);

}  // namespace ntts
