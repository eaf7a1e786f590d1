/*
 * ncgpu.h — C ABI of the MI355X nightcore analysis engine (libncgpu.so).
 *
 * The drop-in boundary of this repository.  The reference
 * (Tealdragon204/nightcore-to-flac-analyzer) is pure Python and has no FFI; each
 * entry point below replaces the reference function (file:line under
 * nightcore_analyzer/) or the librosa call it makes on the hot path, and is
 * bound from Python by ctypes in nightcore-to-flac-analyzer_amd/nightcore_analyzer/_native.py
 * (the binding a maintainer would add is shown in INTEGRATION.md).
 *
 * Conventions
 *   - plain pointers and sizes only; every array pointer is DEVICE memory
 *     (hipMalloc / torch.cuda tensors) unless documented otherwise;
 *   - all work is stream-ordered on the `stream` argument (a hipStream_t; NULL =
 *     the default stream); no entry point synchronises or allocates except
 *     nc_create/nc_destroy, so a sequence of calls can be captured in a hipGraph;
 *   - scratch comes from a caller-owned workspace of `*_workspace_bytes` bytes;
 *   - every call returns 0 on success, < 0 on error; nc_last_error() returns a
 *     thread-local message for the last failure on the calling thread;
 *   - one context per (device, thread); contexts hold only read-only tables.
 *
 * Signals: mono float32 at 22 050 Hz, concatenated in one buffer; windows,
 * chunks and files are addressed by int64 sample offsets into it ("views", as
 * the reference's AudioWindow.audio is a numpy view, io.py:100).
 */
#ifndef NCGPU_H
#define NCGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nc_ctx nc_ctx;

#define NCGPU_ABI_VERSION 6  /* 6: nc_melodia_probe; 5: nc_pcm16_to_f32; 4: nc_melodia_salience; 3: tuning decision margins, nc_xcorr_peak */

int nc_abi_version(void);
const char* nc_last_error(void);

/* Create / destroy a context on `device` (builds the f32 constant tables:
 * twiddles, Hann windows, Slaney mel bank, CQT bases for the 100-value tuning
 * grid, the half-band decimator). */
int nc_create(int device, nc_ctx** out);
/* The same for audio at `sample_rate` Hz (ABI 5; 8000..48000): the mel bank and the tempogram
 * windows are built for that rate, so the per-window stage, the beat tracker and the hop-64 IBI
 * pass follow tempo.py:27-173 at that sr (librosa passes sr through).  The CQT / tuning tables
 * stay at 22 050 Hz: the chroma entry points and the shared tuning frames need nc_create. */
int nc_create_rate(int device, int sample_rate, nc_ctx** out);
int nc_destroy(nc_ctx* ctx);
/* number of compute units seen by the context (256 on MI355X) */
int nc_num_cu(const nc_ctx* ctx);

/* Opt-in per-kernel timing (no reference equivalent; measurement only).
 * on = 1: the dominant kernels are bracketed by HIP events on their stream AND record
 *         their own execution span; on = 2: spans only (no host work per launch, cheap
 *         enough for a timed region); on = 3: events only around the roofline kernels
 *         ("stft_mel", "cqt_low", "cqt_high", "window_tg"), spans for every kernel (the
 *         other kernels' event records are host and queue work a timed region need not
 *         carry); on = 4: the events of on = 3 without spans (the spans' per-workgroup clock
 *         reads and atomics cost the step ~3 %); on = 5: the spans of on = 2 plus marker
 *         spans around the small entry points (nc_energy_gate, nc_collect_valid, nc_pitch_hz,
 *         nc_tempo_prior, nc_bootstrap_ratio, nc_chroma_lag*, nc_window_energy_blocks and the
 *         chroma plan / tail and trim bounds inside the larger ones: two one-thread marker
 *         launches each, timeline diagnosis only); on = 0: off.
 * nc_profile_read(tag) waits for the recorded launches, returns their summed event
 * duration and count, and resets the tag's events.  nc_profile_read_span(tag) returns
 * the summed execution spans (first wave start .. last wave end on the device wall
 * clock: the duration rocprofv3 --kernel-trace reports, without the time a kernel
 * queues behind other streams' work) and resets the tag's spans.  Tags: "stft_mel",
 * "window_tg", "tuning_peaks", "decimate", "cqt_chroma", "trim_blocks", "tempo_beat",
 * "tg_slide", "spectral_frames", "spectral_bins".  Enabling (or disabling) discards
 * pending records.  nc_profile_read_busy (modes 1-3, 5) returns the union of every span
 * recorded since the last read, all tags together (device busy time), the extent from the
 * first start to the last end, and the number of spanned launches, and clears the spans:
 * 1 - busy / extent is the device's idle fraction over those launches. */
int nc_profile_enable(nc_ctx* ctx, int on);
int nc_profile_read(nc_ctx* ctx, const char* tag, double* total_ms, int* launches);
int nc_profile_read_span(nc_ctx* ctx, const char* tag, double* total_ms, int* launches);
int nc_profile_read_busy(nc_ctx* ctx, double* busy_ms, double* extent_ms, int* launches);
/* nc_profile_dump_spans (modes 1-3): every span recorded since the last read, in launch order:
 * the launch's tag index into `tags` (the tag names written '\n'-separated, NUL-terminated, at
 * most tags_cap bytes), its start and end in ms from the earliest start; at most cap spans,
 * *n = how many.  Clears the spans (as nc_profile_read_busy).  Measurement only: the untraced
 * timeline of which kernels run together (tools/concurrency.py). */
int nc_profile_dump_spans(nc_ctx* ctx, char* tags, int tags_cap, int* tag_index, double* start_ms, double* end_ms,
                          int cap, int* n);

/* ---------------------------------------------------------------------------
 * K1a  silence trim — replaces io.strip_silence (io.py:58-79) ->
 *      librosa.effects.trim(y, top_db) (io.py:76).
 * For each file f: samples [file_off[f], file_off[f]+file_len[f]) of `sig`;
 * frame RMS (2048/512, centred, zero pad) -> dB re max -> non-silent frames
 * (> -top_db) -> out_start[f] / out_end[f] (sample indices relative to the file,
 * start = first*512, end = min(len, (last+1)*512); 0/0 for an all-silent file).
 * ------------------------------------------------------------------------- */
size_t nc_trim_workspace_bytes(const int64_t* host_file_len, int n_files);
int nc_trim_bounds(nc_ctx* ctx, const float* sig, const int64_t* file_off, const int64_t* file_len,
                   int n_files, int64_t max_frames, float top_db, int64_t* out_start,
                   int64_t* out_end, void* ws, size_t ws_bytes, void* stream);

/* K1b' window energies from a finished nc_trim_bounds workspace (ABI 5) — replaces
 * io._rms_db (io.py:38-40) for windows of the trimmed files: window w of file
 * win_file[w] (an index into that trim call's files, whose untrimmed offsets are
 * file_off) at sig + win_off[w], win_len samples; energy_out[w] = RMS dB (f64) from
 * the trim's f64 512-sample block sums plus the partial blocks at the window ends.
 * The per-window stage then runs with energy_out = NULL (no per-frame energy). */
int nc_window_energy_blocks(nc_ctx* ctx, const float* sig, const void* trim_ws, int n_files, const int64_t* file_off,
                            const int64_t* win_off, const int* win_file, int n_win, int win_len, double* energy_out,
                            void* stream);

/* ---------------------------------------------------------------------------
 * K1b+K2..K5  per-window stage — replaces io._rms_db (io.py:38-40) and, inside
 * tempo.estimate_tempo (tempo.py:27-77), librosa.onset.onset_strength
 * (tempo.py:44) and the tempogram mean behind beat_track/feature.tempo
 * (tempo.py:45-50, 61-68).
 * Window w = win_len samples at sig + win_off[w] (hop must be 512).
 * Outputs: onset_out[w*T + t] (T = 1 + win_len/512), tg_out[w*acw + k]
 * (acw = 344: mean over frames of the inf-normalised tempogram),
 * energy_out[w] (RMS dB, float64; nullable since ABI 5: then no energy is computed,
 * nc_window_energy_blocks gives it from the trim).  `active` (nullable) skips windows.
 * ------------------------------------------------------------------------- */
size_t nc_window_stage_workspace_bytes(const nc_ctx* ctx, int n_win, int win_len, int hop);
int nc_window_stage(nc_ctx* ctx, const float* sig, const int64_t* win_off, const uint8_t* active,
                    int n_win, int win_len, int hop, float* onset_out, double* tg_out,
                    double* energy_out, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * K6..K8  tempo + beat tracking — replaces librosa.beat.beat_track(onset_envelope,
 * sr, hop_length, start_bpm) as called at tempo.py:45-50 (windows) and
 * tempo.py:159-164 (full signal); with feature.tempo (tempo.py:63) giving the
 * identical tempo, this is all of estimate_tempo after the onset envelope.
 * Sequence s: onset[off[s] .. off[s]+len[s]), tempogram mean tg[s*acw ..].
 * start_bpm: per sequence, or per group when prior_idx != NULL
 * (start = start_bpm[prior_idx[s]]).
 * Outputs: bpm_out (tempo, float64; 0 when the onset envelope is all zero),
 * lag_out (tempogram lag), nbeats_out (beats after trimming; -1 = capacity
 * error), margin_out (nullable: score gap to the runner-up lag),
 * beats_out (nullable: beat frames written at off[s]).
 * Workspace needed only when max_len is too long for LDS (hop-64 signals).
 * ------------------------------------------------------------------------- */
size_t nc_tempo_beats_workspace_bytes(int64_t total_frames);
int nc_tempo_beats(nc_ctx* ctx, const float* onset, const int64_t* off, const int* len, int n_seq,
                   int max_len, const double* tg, int acw, const double* start_bpm,
                   const int* prior_idx, const uint8_t* active, int hop, int trim, double* bpm_out,
                   int* lag_out, int* nbeats_out, double* margin_out, int* beats_out,
                   int64_t total_frames, void* ws, size_t ws_bytes, void* stream);

/* nc tempo prior — pipeline.py:174-183: median of the valid source-window
 * tempos (active and nbeats >= 4) of pair p (windows [src_w0[p], src_w1[p]))
 * times src_len[p]/nc_len[p]; 120 when none is valid. */
int nc_tempo_prior(nc_ctx* ctx, const double* bpm, const int* nbeats, const uint8_t* active,
                   const int* src_w0, const int* src_w1, const int64_t* src_len,
                   const int64_t* nc_len, int n_pairs, double* prior_out, void* stream);

/* tempo.py:165-172 — inter-beat intervals (s) of each beat list, glitches
 * (<= 0.05 s) removed; n_ibi[s] = 0 when fewer than min_ibis remain (None). */
int nc_ibi_from_beats(nc_ctx* ctx, const int* beats, const int64_t* off, const int* nbeats, int n_seq,
                      int hop, int min_ibis, double* ibi_out, int* n_ibi, void* stream);


/* ---------------------------------------------------------------------------
 * K9..K11  CQT chroma — replaces pitch._mean_chroma (pitch.py:55-64) =
 * librosa.feature.chroma_cqt(y, sr=22050, bins_per_octave=36, hop_length=512)
 * .mean(axis=1) for each chunk c = sig[chunk_off[c] .. +chunk_len[c]):
 * tuning estimate (piptrack, 0.01-bin histogram) -> 7-octave CQT (252 bins,
 * octave decimation by the engine's half-band FIR in place of soxr_hq) ->
 * 12-bin chroma (n_chroma = 12: the reference's lag/3 quirk) ->
 * per-frame inf-norm -> mean.  out_chroma[c*12 + k] (f32), out_tuning[c]
 * (f32, bins), out_tuning_idx[c] (nullable; index on the 0.01 grid),
 * out_tuning_margin[c] (nullable; the tuning decision's margin: the argmax bin's
 * residual count minus the runner-up's, 0 on a tie broken by np.argmax's first-index
 * rule, 0 when no peak passes the threshold).
 * total_len = sum of chunk_len; max_chunk_len = max of chunk_len.
 * ------------------------------------------------------------------------- */
size_t nc_chroma_workspace_bytes(const nc_ctx* ctx, int n_chunks, int64_t total_len);
int nc_chroma_mean(nc_ctx* ctx, const float* sig, const int64_t* chunk_off, const int64_t* chunk_len,
                   int n_chunks, int64_t total_len, int64_t max_chunk_len, float* out_chroma,
                   float* out_tuning, int* out_tuning_idx, int* out_tuning_margin, void* ws, size_t ws_bytes,
                   void* stream);

/* Where nc_chroma_mean leaves its intermediates in the caller's workspace (host only,
 * launches nothing; for inspection and tests, no reference equivalent).  The launcher
 * carves its workspace through the same function, so the answer cannot drift from it.
 * Fills out[0 .. 26) (cap >= 26) and returns 26, or -2 on a bad argument:
 *   [0]  entries written (26)
 *   byte offsets into ws, each section 256-byte aligned (n = n_chunks):
 *   [1]  oct_off    int64[n][7]  float offset of level o of chunk c inside ws_oct
 *                   (o = 0: -1, level 0 is the chunk itself inside sig)
 *   [2]  oct_len    int64[n][7]  length of level o: L_0 = chunk_len, L_{o+1} = ceil(L_o / 2)
 *   [3]  n_frames   int32[n]     CQT frames T = min over o of 1 + L_o / (512 >> o)
 *   [4]  n_tframes  int32[n]     tuning STFT frames 1 + chunk_len / 512
 *   [5]  chunk_npk  int32[n]     piptrack peaks in the chunk's list (nc_chroma_mean_shared
 *                                counts into the caller's array instead)
 *   [6]  tuning_idx int32[n]     used only when out_tuning_idx is NULL
 *   [7]  tf_base    int64[n+1]   prefix sum of n_tframes
 *   [8]  oct_base   int64[n+1]   prefix sum of the chunks' octave-buffer floats
 *   [9]  ws_oct     float[]      decimated levels 1..6, y_{o+1} = sqrt(2) halfband(y_o)[::2];
 *                                each level padded to a multiple of 64 floats (the padding
 *                                is not written)
 *   [10] peak_pitch float[]      chunk c's peaks at [tf_base[c] * kPeakSlots ..
 *   [11] peak_mag   float[]      + chunk_npk[c]), in no particular order (appended at an
 *                                atomic position); peak_mag is 2x piptrack's magnitude.
 *                                nc_chroma_mean_shared uses the caller's lists instead
 *   [12] partial    double[]     per-tile sums of the normalised chroma (cqt_tail)
 *   [13] tp_base    int64[n+1]   prefix of the tuning frames the chain itself computes
 *   [14] xmax       float[]      max |level 0| per decimation tile of chunk c, at slot
 *                                c + oct_off[c][3] / 256 + tile
 *   [15] gpart      float[][7][12]  row tf_base[c] + t (t < n_frames[c]) holds frame t's
 *                                chroma partial sums per octave: gpart[row][k][j] is the sum
 *                                of |C| over CQT bins 36 k + {3j - 1, 3j, 3j + 1} (3j - 1
 *                                wraps to 36 k + 35 for j = 0), k = 0 the lowest octave
 *                                (bins 0..35, from level 6) .. k = 6 the highest (bins
 *                                216..251, from level 0, the chunk itself); column j is
 *                                chroma j (0 = C, 1 = C#, .. 11 = B).  The device's octave
 *                                index o (levels, oct_ex) is 6 - k
 *   [16] oct_ex     int32[n][7]  f16 split exponent of level o: the CQT scales the level's
 *                                samples by 2^oct_ex, 0 for a silent chunk
 *   [17] bytes carved (nc_chroma_workspace_bytes is this plus slack)
 *   constants: [18] D3_TILE level-(base + 3) outputs per decimation workgroup (8 D3_TILE
 *   level-0 samples for levels 1-3, 64 D3_TILE for levels 4-6), [19] kPeakSlots peak slots
 *   per tuning frame, [20] CH_FR frames per tile of the CQT of levels 3-6, [21] C2_FR and
 *   [22] C2_NW frames per tile and tiles per workgroup of the CQT of levels 0-2, [23] CM_FR
 *   frames per tail tile, [24] kHalfbandK (the decimator has 2 kHalfbandK + 1 taps).
 *   [25] head       float[n][4], then int64[n]: the first four samples of every chunk (zeros
 *                   past its end) and where the CQT of level 0 reads each chunk, in floats from
 *                   sig: chunk_off[c], or for a chunk under 4 samples the distance of its head
 *                   slot from sig, so that no 16-byte load passes the end of the caller's buffer */
int nc_chroma_workspace_layout(const nc_ctx* ctx, int n_chunks, int64_t total_len, int64_t* out, int cap);

/* ---------------------------------------------------------------------------
 * K9-K11 with shared tuning frames (optional fusion; same results as the pair
 * nc_window_stage + nc_chroma_mean).  The first tp_frames tuning frames (2048 / 512,
 * centred) of a 20 s chunk that starts where a 10 s window starts are that window's
 * own STFT frames: same samples, same zero padding on the left, none on the right
 * while t * 512 + 1024 <= win_len (tp_frames = 429 for 10 s windows).
 * nc_window_stage_tuning = nc_window_stage that also runs estimate_tuning's piptrack
 * (pitch.py:58 -> librosa.estimate_tuning) on those frames: win_chunk[w] = the chunk
 * window w starts (or -1), chunk_tf_base[c] = sum_{q<c} (1 + chunk_len[q] / 512) (the
 * chunk's slot base in the peak lists, in units of 192 slots), peak_pitch / peak_mag =
 * chunk_tf_base[n] * 192 floats each (peak_mag holds 2x piptrack's magnitude, exactly:
 * only its median and comparisons are consumed), chunk_npk[n] zeroed by the caller.  If
 * stft_done_event (a hipEvent_t) is given it is recorded once the peaks are written.
 * nc_chroma_mean_shared = nc_chroma_mean on the same peak lists: tuning frames
 * t < tf_skip[c] are not recomputed (tf_skip_total = sum of tf_skip, host value), the
 * counts are not zeroed, and the stream waits for wait_event before the tuning select.
 * ------------------------------------------------------------------------- */
int nc_window_stage_tuning(nc_ctx* ctx, const float* sig, const int64_t* win_off, const uint8_t* active,
                           int n_win, int win_len, int hop, float* onset_out, double* tg_out,
                           double* energy_out, const int* win_chunk, const int64_t* chunk_tf_base,
                           int tp_frames, float* peak_pitch, float* peak_mag, int* chunk_npk,
                           void* stft_done_event, void* ws, size_t ws_bytes, void* stream);
int nc_chroma_mean_shared(nc_ctx* ctx, const float* sig, const int64_t* chunk_off, const int64_t* chunk_len,
                          int n_chunks, int64_t total_len, int64_t max_chunk_len, float* out_chroma,
                          float* out_tuning, int* out_tuning_idx, int* out_tuning_margin, const int* tf_skip,
                          int64_t tf_skip_total,
                          float* peak_pitch, float* peak_mag, int* chunk_npk, void* wait_event, void* ws,
                          size_t ws_bytes, void* stream);
/* pitch._cyclic_xcorr_peak (pitch.py:67-85): lag_out[p] = wrapped argmax_k
 * dot(chroma[src_idx[p]], roll(chroma[nc_idx[p]], -k)), in [-5, 6]. */
int nc_chroma_lag(nc_ctx* ctx, const float* chroma, const int* src_idx, const int* nc_idx, int n_pairs,
                  int* lag_out, void* stream);
/* nc_chroma_lag plus margin_out[p] = (best - second best xcorr) / |best|: how far the
 * lag decision is from a tie (no reference equivalent; diagnostics). */
int nc_chroma_lag_margin(nc_ctx* ctx, const float* chroma, const int* src_idx, const int* nc_idx, int n_pairs,
                         int* lag_out, double* margin_out, void* stream);
/* pitch._cyclic_xcorr_peak (pitch.py:67-85) for vectors of any length n >= 1: pair p is
 * src[p*n .. p*n+n) against nc[p*n .. p*n+n); lag_out[p] = argmax_k dot(src, roll(nc, -k))
 * (first maximum, first NaN wins as np.argmax), minus n when it exceeds n / 2. */
int nc_xcorr_peak(nc_ctx* ctx, const float* src, const float* nc, int n, int n_pairs, int* lag_out, void* stream);

/* ---------------------------------------------------------------------------
 * device glue between the kernels (so a batch needs no host round trip)
 * nc_energy_gate   io.energy_gate (io.py:115-126) per group of windows
 *                  [w0[g], w1[g]): active[w] = energy_db[w] >= max + threshold_db
 * nc_collect_valid consensus._valid (consensus.py:236-240) of the per-window
 *                  tempo lists: in window order, values of windows that are
 *                  active, have nbeats >= min_beats (tempo.py:54-55) and a finite
 *                  positive bpm -> out_values[w0[g] + i], count out_n[g]
 * nc_pitch_hz      pitch.py:95,161-164: shift = lag/3.0, nc_hz = 440*2^(shift/12),
 *                  src_hz = 440
 * ------------------------------------------------------------------------- */
/* io._rms_db (io.py:38-40) alone, for windows sig[win_off[w] .. +win_len) */
int nc_window_energy(nc_ctx* ctx, const float* sig, const int64_t* win_off, int n_win, int win_len,
                     double* energy_out, void* stream);
int nc_energy_gate(nc_ctx* ctx, const double* energy_db, const int* w0, const int* w1, int n_groups,
                   double threshold_db, uint8_t* active_out, void* stream);
int nc_collect_valid(nc_ctx* ctx, const double* bpm, const int* nbeats, const uint8_t* active,
                     const int* w0, const int* w1, int n_groups, int min_beats, double* out_values,
                     int* out_n, void* stream);
int nc_pitch_hz(nc_ctx* ctx, const int* lags, int n, double* shift_out, double* nc_hz, double* src_hz,
                void* stream);

/* ---------------------------------------------------------------------------
 * K12  bootstrap ratio of medians — replaces consensus._bootstrap_ratio
 * (consensus.py:243-267), consensus.compute_ibi_ratio (consensus.py:270-312)
 * and the chunk-shift bootstrap of pitch.estimate_pitch_chroma
 * (pitch.py:143-150).  Job j draws A = values[a_off[j] .. +a_n[j]) first and
 * B = values[b_off[j] .. +b_n[j]) second (b_off/b_n NULL: single array) with
 * numpy Generator(PCG64) choice(replace=True) semantics, bit-exact:
 * seed[j*4 .. +4] = PCG64 {state_hi, state_lo, inc_hi, inc_lo} of
 * np.random.default_rng(seed).  boot[i] = median(A*)/median(B*) (median(A*));
 * point = median(A)/median(B); CI = numpy 'linear' percentiles given as
 * (virtual index, gamma) pairs for the low and high quantile.  Jobs with
 * a_n < min_n (or b_n < min_n) yield NaN (the reference's MIN_VALID gate).
 * Workspace: job j uses job_cap[j] (>= a_n + b_n) values at byte offset
 * job_ws_off[j]; size each with nc_bootstrap_job_bytes(cap, n_boot).
 * ------------------------------------------------------------------------- */
size_t nc_bootstrap_job_bytes(int cap, int n_boot);
int nc_bootstrap_ratio(nc_ctx* ctx, const double* values, const int64_t* a_off, const int* a_n,
                       const int64_t* b_off, const int* b_n, int n_jobs, int n_boot,
                       const uint64_t* seed, double idx_lo, double gamma_lo, double idx_hi,
                       double gamma_hi, int min_n, double* point_out, double* lo_out, double* hi_out,
                       double* boot_out, const int64_t* job_ws_off, const int* job_cap, void* ws,
                       size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * hop-64 IBI pass, part 1 — librosa.onset.onset_strength(y, sr, hop_length=hop)
 * over whole files (tempo.py:158): file f = sig[file_off[f] .. +file_len[f]),
 * onset_out at frame_base[f] (frame_base_out[n_files+1], written here:
 * prefix of 1 + file_len/hop).  total_frames = sum(1 + file_len/hop).
 * ------------------------------------------------------------------------- */
size_t nc_ibi_onset_workspace_bytes(const nc_ctx* ctx, int n_files, int64_t total_frames);
int nc_ibi_onset(nc_ctx* ctx, const float* sig, const int64_t* file_off, const int64_t* file_len,
                 int n_files, int64_t total_frames, int hop, float* onset_out,
                 int64_t* frame_base_out, void* ws, size_t ws_bytes, void* stream);
/* part 2 — the tempogram mean (win_length = ac_size*sr/hop, 2756 at hop 64)
 * that beat_track argmaxes (tempo.py:159), streamed instead of materialised:
 * tg_out[f*acw + k].  total_frames = frame_base[n_files]; max_frames = the
 * largest per-file frame count (sizes the tile grid). */
size_t nc_ibi_tempogram_workspace_bytes(const nc_ctx* ctx, int n_files, int64_t total_frames, int max_frames,
                                        int hop);
int nc_ibi_tempogram(nc_ctx* ctx, const float* onset, const int64_t* frame_base, int n_files,
                     int64_t total_frames, int max_frames, int hop, double* tg_out, void* ws, size_t ws_bytes,
                     void* stream);
/* The same pass split over ranks (window-sharded runs); one rank's
 * share of file f is frames [t0[f], t1[f]) and tempogram tiles [b0[f], b1[f]) (2048 frames
 * each); t0 / t1 / b0 / b1 are device int64 arrays.
 * nc_ibi_mel_range:   the mel dB rows the onsets of [t0, t1) need (STFT frames
 *                     [t0 - pad, t1 - pad + 1) within the file, pad = 1 + 1024 / hop) into ws,
 *                     and max_out[f] = their largest dB value (-inf for none): this rank's
 *                     share of power_to_db's top_db reference (C2: all-reduce MAX).
 *                     total_rows = the host's count of those rows over all files.
 * nc_ibi_onset_range: onset_out[obase[f] + t - t0[f]] for t in [t0[f], t1[f]) (obase =
 *                     prefix of t1 - t0; total_out = its sum) against the file's global
 *                     maximum gmax[f]; ws and total_rows as in the nc_ibi_mel_range call.
 *                     (C4: the segments are gathered into each file's full onset.)
 * nc_ibi_tempogram_tiles:  partial rows slab[(f * n_tblk + b) * N + k] of tiles
 *                     b in [b0[f], b1[f]) from the FULL onset (n_tblk = ceil(max_frames / 2048),
 *                     N = tempogram window); ws sized by nc_ibi_tempogram_workspace_bytes.
 * nc_ibi_tempogram_reduce: tg_out[f * N + k] = (sum over b of slab rows, in order) / T_f
 *                     once every tile's row is in slab (C3: the rows are gathered) -- the
 *                     same bits as nc_ibi_tempogram. */
size_t nc_ibi_range_workspace_bytes(const nc_ctx* ctx, int n_files, int64_t total_rows);
int nc_ibi_mel_range(nc_ctx* ctx, const float* sig, const int64_t* file_off, const int64_t* file_len,
                     int n_files, const int64_t* t0, const int64_t* t1, int hop, int64_t total_rows,
                     float* max_out, void* ws, size_t ws_bytes, void* stream);
int nc_ibi_onset_range(nc_ctx* ctx, int n_files, const int64_t* t0, int hop, int64_t total_out,
                       const float* gmax, float* onset_out, void* ws, int64_t total_rows, void* stream);
int nc_ibi_tempogram_tiles(nc_ctx* ctx, const float* onset, const int64_t* frame_base, int n_files,
                           int64_t total_frames, int max_frames, int hop, const int64_t* b0, const int64_t* b1,
                           double* slab, void* ws, size_t ws_bytes, void* stream);
int nc_ibi_tempogram_reduce(nc_ctx* ctx, const double* slab, const int64_t* frame_base, int n_files,
                            int max_frames, int hop, double* tg_out, void* stream);

/* ---------------------------------------------------------------------------
 * K13  windowed waveform cross-correlation — the search loop of
 * xcorr.estimate_speed_xcorr (xcorr.py:109-160).  The caller plans the
 * reference's integer geometry: n_items dot products of `win` samples between
 * sig[item_a[i]..] and sig[item_b[i]..]; job j owns windows [w0[j], w1[j]);
 * window w has its self item win_self[w] (a.a), candidate items
 * [cand0[w], cand1[w]) whose b positions are pb[item], its a position pa[w]
 * and default exp_pb[w].  Outputs ratio_out[j] (np.polyfit slope) and
 * quality_out[j] (median normalised correlation); (1, 0) with < 3 matches.
 * A job may own any number of windows (the reference's n_windows is unbounded).
 * scratch: dot/sqb = 2 * n_items doubles (caller-owned device memory), holding
 * nothing of use afterwards: each window's self item must be its own (shared
 * by no other window or job), because its two slots are reused for that
 * window's best correlation and b position once its a.a has been read.
 * ------------------------------------------------------------------------- */
int nc_xcorr_search(nc_ctx* ctx, const float* sig, const int64_t* item_a, const int64_t* item_b,
                    int n_items, int win, double* dot, double* sqb, const int* w0, const int* w1,
                    const int* win_self, const int* cand0, const int* cand1, const int64_t* pa,
                    const int64_t* pb, const int64_t* exp_pb, int n_jobs, double* ratio_out,
                    double* quality_out, void* stream);

/* ---------------------------------------------------------------------------
 * intro offset of pipeline.run(auto_align=True) — xcorr.find_content_offset
 * (xcorr.py:165-259; called at pipeline.py:111-125) for n_pairs (src, nc)
 * pairs of 22050 Hz signals (sig[src_off[p] ..], src_len[p] samples; likewise
 * nc): 2:1 resample to 11025 Hz, RMS envelopes (frame 2048, hop 512), for each
 * of n_speeds candidate speeds (device f64, the reference's np.linspace(1.03,
 * 1.5, 30)) the nc envelope stretched to int(len / speed) frames by np.interp
 * and correlated with the first max_offset_frames + 1 lags of the src envelope
 * (int(120 / (512 / 11025)) = 2583 in the reference); the cosine score of each
 * speed's first argmax decides, first best wins.  Outputs per pair: peak lag
 * (offset_sec = peak * 512 / 11025), speed index (-1: no speed searchable,
 * the reference then returns (0.0, (lo + hi) / 2)) and the score.
 * total_len = sum of all 2 n_pairs lengths, max_len = the longest (grid and
 * workspace sizing); size ws with nc_align_workspace_bytes.
 * ------------------------------------------------------------------------- */
size_t nc_align_workspace_bytes(const nc_ctx* ctx, int n_pairs, int n_speeds, int64_t total_len,
                                int64_t max_len, int max_offset_frames);
int nc_align_offsets(nc_ctx* ctx, const float* sig, const int64_t* src_off, const int64_t* src_len,
                     const int64_t* nc_off, const int64_t* nc_len, int n_pairs, const double* speeds,
                     int n_speeds, int max_offset_frames, int64_t total_len, int64_t max_len,
                     int* peak_out, int* speed_idx_out, double* score_out, void* ws, size_t ws_bytes,
                     void* stream);

/* ---------------------------------------------------------------------------
 * S1  spectral statistics — replaces, inside spectral.analyze (spectral.py:38-103),
 *     librosa.feature.spectral_centroid (:54), spectral_rolloff(roll_percent) (:55-57),
 *     feature.rms (:59, :76), the |stft| band means (:63-74) and
 *     amplitude_to_db(|stft|, ref=np.max) averaged over time (:87-88).
 * File f = file_len[f] samples at sig + file_off[f], at its own sample rate (the
 * reference loads with sr=None, :52).  STFT 2048 / hop 512, periodic Hann, centred,
 * zero pad: T_f = 1 + file_len[f] / 512 frames, frame_base[f] = sum_{q<f} T_q
 * (device, n_files + 1 entries; total_frames = frame_base[n_files], max_frames =
 * max T_f).  bin_hz[f] = np.fft.rfftfreq(2048, 1/sr)[1] (f64, device);
 * band_bins[f*10 + 2b], [f*10 + 2b + 1] = the [lo, hi) bins of band b's mask
 * (freqs >= lo_hz) & (freqs < hi_hz) for the bands 20-80, 80-250, 250-2000,
 * 2000-6000, 6000-20000 Hz.
 * Outputs: rms_out[frame_base[f] + t] = frame RMS (f32); stats_out[f*12 + i] =
 * {sum_t centroid_t, sum_t rolloff_t (Hz), 5 x sum_t sum_{k in band} |S|, max |S|,
 * mean(rms), var(rms), np.percentile(rms, 75), mean(diff(rms[rms > p75]))};
 * bin_db_out[f*1025 + k] = sum_t max(dB(|S|^2) - dB(ref^2), -80).  The host
 * divides by T_f (and by the band bin counts) and thresholds the bin means.
 * Size ws with nc_spectral_workspace_bytes.
 * ------------------------------------------------------------------------- */
size_t nc_spectral_workspace_bytes(int64_t total_frames, int n_files, int64_t max_frames);
int nc_spectral_stats(nc_ctx* ctx, const float* sig, const int64_t* file_off, const int64_t* file_len,
                      const int64_t* frame_base, const double* bin_hz, const int* band_bins, int n_files,
                      int64_t total_frames, int64_t max_frames, float roll_percent, float* rms_out,
                      double* stats_out, double* bin_db_out, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * R1  load-time resampler — replaces the resample inside io.load_audio
 *     (io.py:44-55: librosa.load(path, sr=22050) -> soxr_hq) for files that are
 *     not at 22 050 Hz.  libsoxr is absent and cannot be bit-matched; the engine's
 *     stand-in is scipy.signal.resample_poly(x, up, down) (Kaiser(5.0) FIR,
 *     constant zero padding), reproduced bit for bit in f64.  For each file f:
 *     y[out_off[f] + m] = upfirdn(h, x[in_off[f] ..], up, down)[m + pre_remove]
 *     (float), m < out_len[f] = ceil(in_len[f] up / down); max_out = max out_len.
 *     h (device f64, h_len = a multiple of up) is resample_poly's filter:
 *     firwin(20 max(up,down) + 1, 1/max(up,down), ('kaiser', 5)) * up, with its
 *     leading / trailing zero padding; pre_remove = resample_poly's n_pre_remove.
 *     All files of one call share (up, down, h).
 * ------------------------------------------------------------------------- */
int nc_resample_poly(nc_ctx* ctx, const float* x, const int64_t* in_off, const int64_t* in_len, int n_files,
                     float* y, const int64_t* out_off, const int64_t* out_len, int64_t max_out,
                     const double* h, int h_len, int up, int down, int64_t pre_remove, void* stream);

/* -------------------------------------------------------------------------
 * R1b 16-bit PCM upload — replaces the int16 -> float32 scaling inside
 *     io.load_audio (io.py:44-55: librosa.load -> soundfile, sample k -> k / 32768)
 *     for mono 16-bit WAV files: the host uploads the stored 2-byte samples and
 *     y[i] = x[i] / 32768 (exact in f32) is computed in HBM.  x and y 16-byte
 *     aligned, n samples.  (ABI 5)
 * ------------------------------------------------------------------------- */
int nc_pcm16_to_f32(nc_ctx* ctx, const int16_t* x, int64_t n, float* y, void* stream);

/* -------------------------------------------------------------------------
 * R2  speed render — replaces the `sox SRC DST speed F` the reference's workflow
 *     shells out to (workflow.py:108-118) with an arbitrary-ratio band-limited
 *     resampler.  PARITY UNPINNED: sox is not installed and the reference holds no
 *     resampler; the definition is this project's own:
 *       Q = 1e6, Z = 32, BETA = 10.06, ROLL = 0.9, P = round(F Q), 0.25 <= F <= 4,
 *       n_out = ceil(n Q / P), c = ROLL min(1, Q / P),
 *       t_m = (m P div Q) + ((m P mod Q) / Q),
 *       h(u) = c sinc(c u) I0(BETA sqrt(1 - (c u / Z)^2)) / I0(BETA), |c u| < Z,
 *       y[m] = sum_j x[j] h(t_m - j), x zero outside [0, n).
 *
 * nc_speed_out_len (host only, no context): *p_out = P (nullable) and
 *     n_out[f] = ceil(n_in[f] Q / P) for n_files host lengths; -2 when F is outside
 *     [0.25, 4].  The renderer uses the same formula on the device.
 * nc_speed_render: file f's y[out_off[f] + m], m < n_out(in_len[f]), and
 *     peak[f] = max_m |y[m]| (0 for an empty file) in one launch; files of one call
 *     share p = P.  in_off / in_len / out_off: device int64 [n_files] (samples);
 *     max_out = the largest n_out; peak: device float [n_files].  The filter is
 *     read from a 512-point-per-zero-crossing table by linear interpolation and
 *     summed in f32: within 1e-5 max|x| of the definition.  No workspace, no host
 *     synchronisation.
 * nc_f32_to_pcm16: q[out_off[f] + i out_stride] = clamp(rint(x[in_off[f] + i] 32768),
 *     -32768, 32767) (round half to even), i < in_len[f]; out_stride = channels
 *     interleaves the channels of one WAV file; clipped[f] (device int) = samples
 *     whose rounded value fell outside the 16-bit range.  max_len = largest in_len.
 * ------------------------------------------------------------------------- */
int nc_speed_out_len(double factor, const int64_t* n_in, int n_files, int64_t* p_out, int64_t* n_out);
int nc_speed_render(nc_ctx* ctx, const float* x, const int64_t* in_off, const int64_t* in_len, int n_files,
                    int64_t p, float* y, const int64_t* out_off, int64_t max_out, float* peak, void* stream);
int nc_f32_to_pcm16(nc_ctx* ctx, const float* x, const int64_t* in_off, const int64_t* in_len, int n_files,
                    int64_t max_len, int16_t* q, const int64_t* out_off, int64_t out_stride, int* clipped,
                    void* stream);

/* -------------------------------------------------------------------------
 * R3  true-peak limiter — replaces the `ffmpeg -af alimiter=limit=L:attack=5:
 *     release=50:level=disabled` the reference's loudness.apply_true_peak_limiter
 *     shells out to (loudness.py:86-134), channels linked, no make-up gain.
 *     PARITY UNPINNED: ffmpeg is not installed and the reference holds no limiter;
 *     the definition is this project's own (tests/limiter_ref.py).
 *     For the channels x_c[n], n < N, of one file (zero outside),
 *     L = 10^(limit_db / 20), Wa = attack, Wr = release (samples), beta = exp(-1 / Wr):
 *       h(u) = sinc(u) I0(9 sqrt(1 - (u / 12)^2)) / I0(9), |u| < 12,
 *       x_c(n + k/4) = sum_{i = -11..12} x_c[n + i] h(k/4 - i), k = 1, 2, 3,
 *       t[n] = max_c max_k |x_c(n + k/4)|, p[n] = max(max_c |x_c[n]|, t[n-1], t[n]),
 *       r[n] = min(1, L / p[n]) (1 where p = 0 and outside the file),
 *       hA[n] = min_{0 <= i < Wa} r[n + i], a[n] = (1 / Wa) sum_{0 <= i < Wa} hA[n - i],
 *       d[n] = max(1 - a[n], beta d[n-1]), d[-1] = 0, g[n] = 1 - d[n],
 *       y_c[n] = clamp(x_c[n] g[n], -L, L) with L rounded to float.
 *
 * A file is a group of consecutive signals of one length (its channels):
 *     file f = signals file_first[f] .. file_first[f + 1] - 1, file_first[0] = 0
 *     (device int [n_files + 1]); sig_off / sig_len: device int64 per signal
 *     (samples).  host_len / host_first are the HOST's copies of sig_len /
 *     file_first, read by the argument checks and the launch geometry only.
 *     x (and y) 16-byte aligned.  Files of different lengths and channel counts
 *     share one call; n_files <= 65535.
 * nc_limiter_ws_bytes (host only, no context): the workspace bytes of files of
 *     n_frames[f] frames each, and ws_off[f] (host, nullable) = file f's byte
 *     offset in it, to be handed to nc_true_peak_limit as a device array.
 * nc_true_peak: true_peak[f] = max_n p[n] (device float, 0 for an empty file), one
 *     launch, no workspace.
 * nc_true_peak_limit: y[y_off[s] + n] for every signal s (y = x with y_off = sig_off
 *     limits in place), true_peak[f] as above, peak_out[f] = max |y| (device float)
 *     and limited[f] = #{n : (float)g[n] < 1} (device int), in four launches whatever
 *     the lengths; no host synchronisation, no allocation; deterministic run to run.
 *     Returns -2 (nc_last_error) when limit_db > 0, attack outside 1 .. 2048,
 *     release < 1, a file without channels, channels of unequal length, or a
 *     workspace below nc_limiter_ws_bytes.  r is computed in f32 (3 x 24 taps), the
 *     box mean exactly in 64-bit fixed point, the release in f64: g within 1e-4
 *     of the f64 definition (measured: DESIGN.md §2).
 * ------------------------------------------------------------------------- */
size_t nc_limiter_ws_bytes(const int64_t* n_frames, int n_files, int64_t* ws_off);
int nc_true_peak(nc_ctx* ctx, const float* x, const int64_t* sig_off, const int64_t* sig_len, const int* file_first,
                 const int64_t* host_len, const int* host_first, int n_files, float* true_peak, void* stream);
int nc_true_peak_limit(nc_ctx* ctx, const float* x, const int64_t* sig_off, const int64_t* sig_len,
                       const int* file_first, const int64_t* host_len, const int* host_first, int n_files,
                       double limit_db, int attack, int release, float* y, const int64_t* y_off, float* true_peak,
                       float* peak_out, int* limited, void* ws, const int64_t* ws_off, size_t ws_bytes,
                       void* stream);

/* -------------------------------------------------------------------------
 * R4  phase-vocoder time stretch — with nc_speed_render at the same ratio it
 *     replaces the `rubberband --pitch S` the reference's workflow shells out to
 *     (workflow.py:121-131): a pitch shift by S semitones, duration kept.
 *     PARITY UNPINNED: rubberband is not installed and the reference holds no
 *     pitch shifter; the definition is this project's own (DESIGN.md §4,
 *     tests/pvoc_ref.py).  Plain phase vocoder: no transient detection, no phase
 *     locking, channels independent.  N = 2048, Hs = 512, Q = 1e6,
 *     W[j] = 0.5 - 0.5 cos(2 pi j / N), P = round(2^(S/12) Q), |S| <= 12; for one
 *     channel x[0..n) (zero outside), every integer division a floor division:
 *       Ns = ceil(n P / Q), K = ceil(Ns / Hs) + 3 (0 when n = 0),
 *       u_k = ((k - 1) Hs Q) div P,
 *       A_k = rfft(x[u_k - N/2 + i] W[i]), B_k = the frame Hs samples earlier,
 *       mag_k = |A_k|, empty_k = every x[i], u_k - N/2 < i < u_k + N/2, is +-0,
 *       reset_k = (k == 0) or empty_{k-1}, ph(z) = z / |z|, (1, 0) at |z| = 0 / inf,
 *       V_k = ph(A_k) on a reset frame, else ph(A_k conj(B_k)),
 *       Phi_k = V_k on a reset frame, else ph(Phi_{k-1} V_k),
 *       f_k[i] = irfft(mag_k Phi_k)[i] W[i] 2/3,
 *       s[m] = sum_{k = j..j+3} f_k[m - (k - 3) Hs], j = m div Hs, m < Ns (ascending k).
 *     The shifted signal is nc_speed_render(s, p = P)[0..n).
 *
 * Frames of all files are numbered consecutively: frame g = frame_base[f] + k.
 *     mag: device float [total_frames][1025]; v / phi: device float
 *     [total_frames][1025][2] (re, im); empty: device uint8 [total_frames];
 *     in_off / in_len / out_off: device int64 [n_files] (samples); frame_base:
 *     device int64 [n_files + 1].  Files of different lengths share one call,
 *     n_files <= 65535, n = 0 is legal (no frames, peak 0).  Every entry returns -2
 *     (nc_last_error) on an argument error; none allocates or synchronises the
 *     host; every sum runs in a fixed order: bit-identical run to run and batch
 *     to single.
 * nc_pv_plan (host only, no context): for p = P and n_files host lengths,
 *     ns_out[f] = Ns, k_out[f] = K, frame_base[f] (host, [n_files + 1]: to be
 *     handed on as a device array), and the workspace of nc_pv_stretch:
 *     ws_off[0..5] = byte offsets of mag, v, phi, the frame buffer
 *     ([total_frames][2048] float), empty and the scan workspace, *ws_bytes the
 *     total.  Every output is nullable.  -2 outside 500000 <= p <= 2000000.
 * nc_pv_analyze: mag, v and empty of every frame (one launch).
 * nc_pv_scan: phi from v and empty (three launches: tiles of 64 frames multiplied
 *     up in f64, the carries over the tile aggregates, the apply pass).
 *     max_frames = the largest K; ws: at least nc_pv_scan_ws_bytes(total_frames,
 *     n_files) bytes (host only; the region nc_pv_plan puts at ws_off[5]), 16-byte
 *     aligned.
 * nc_pv_synth: s[out_off[f] + m], m < Ns(in_len[f]), and peak[f] = max_m |s[m]|
 *     (device float, 0 for an empty file) from mag and phi (two launches: the
 *     windowed inverse FFTs into `frames`, frames_bytes >= 8192 total_frames, then
 *     the four-frame gather).  max_ns = the largest Ns.
 * nc_pv_stretch: the three stages over one workspace laid out by nc_pv_plan
 *     (ws_off: the HOST array nc_pv_plan filled), six launches whatever the lengths.
 * ------------------------------------------------------------------------- */
int nc_pv_plan(int64_t p, const int64_t* n_in, int n_files, int64_t* ns_out, int64_t* k_out, int64_t* frame_base,
               int64_t* ws_off, size_t* ws_bytes);
size_t nc_pv_scan_ws_bytes(int64_t total_frames, int n_files);
int nc_pv_analyze(nc_ctx* ctx, const float* x, const int64_t* in_off, const int64_t* in_len,
                  const int64_t* frame_base, int n_files, int64_t total_frames, int64_t p, float* mag, float* v,
                  uint8_t* empty, void* stream);
int nc_pv_scan(nc_ctx* ctx, const float* v, const uint8_t* empty, const int64_t* frame_base, int n_files,
               int64_t total_frames, int64_t max_frames, float* phi, void* ws, size_t ws_bytes, void* stream);
int nc_pv_synth(nc_ctx* ctx, const float* mag, const float* phi, const int64_t* in_len, const int64_t* frame_base,
                int n_files, int64_t total_frames, int64_t p, int64_t max_ns, void* frames, size_t frames_bytes,
                float* s, const int64_t* out_off, float* peak, void* stream);
int nc_pv_stretch(nc_ctx* ctx, const float* x, const int64_t* in_off, const int64_t* in_len,
                  const int64_t* frame_base, int n_files, int64_t total_frames, int64_t max_frames, int64_t p,
                  int64_t max_ns, float* s, const int64_t* out_off, float* peak, void* ws, const int64_t* ws_off,
                  size_t ws_bytes, void* stream);

/* -------------------------------------------------------------------------
 * Identity phase locking with linked channels for the stretch above (opt-in;
 * DESIGN.md section 4, "Phase locking"; tests/pvoc_lock_ref.py).  Same
 * conventions: device pointers unless stated, 0 / -1 / -2, no allocation, no
 * host synchronisation, fixed launch counts, bit-identical run to run and
 * batch to single.
 * nc_pv_analyze_u: nc_pv_analyze plus u[frame][1025][2] = ph(A) (one launch);
 *     mag, v and empty are bit-identical to nc_pv_analyze's.  v is nullable here:
 *     the frames Hs earlier are then not transformed (a linked channel needs
 *     mag and u only).
 * nc_pv_lock: owner[frame][1025] (uint16, nullable) and the locked scan phi from
 *     mag, u, v and empty (four launches: peaks / owners / M per frame, then the
 *     tile, carry and apply passes of the scan with a gather).  max_frames = the
 *     largest K; ws: at least nc_pv_lock_ws_bytes(total_frames, n_files) bytes
 *     (host only), 16-byte aligned.
 * nc_pv_mid_sum: mid[mid_off[g] + i] = ((x_0[i] + x_1[i]) + ...) in float32 over
 *     the channels group_first[g] .. group_first[g + 1] - 1 of group g (one
 *     launch).  host_len / host_first: HOST copies of sig_len / group_first;
 *     -2 when the channels of a group differ in length.
 * nc_pv_rotate: phi of every channel frame from its group's locked scan psi and
 *     analysis phasors u_mid (rows laid out by mid_base[groups + 1], the frame
 *     bases of the sums) and the channel's own u (rows by frame_base):
 *     ph(psi u conj(u_mid)) in f64; a group of one channel copies psi (one launch).
 * The locked stretch is nc_pv_analyze_u, nc_pv_lock and nc_pv_synth for
 * unlinked files (7 launches), and nc_pv_mid_sum, nc_pv_analyze_u of the
 * channels and of the sums, nc_pv_lock of the sums, nc_pv_rotate and
 * nc_pv_synth for linked groups (10 launches).
 * ------------------------------------------------------------------------- */
int nc_pv_analyze_u(nc_ctx* ctx, const float* x, const int64_t* in_off, const int64_t* in_len,
                    const int64_t* frame_base, int n_files, int64_t total_frames, int64_t p, float* mag, float* v,
                    uint8_t* empty, float* u, void* stream);
size_t nc_pv_lock_ws_bytes(int64_t total_frames, int n_files);
int nc_pv_lock(nc_ctx* ctx, const float* mag, const float* u, const float* v, const uint8_t* empty,
               const int64_t* frame_base, int n_files, int64_t total_frames, int64_t max_frames, float* phi,
               uint16_t* owner, void* ws, size_t ws_bytes, void* stream);
int nc_pv_mid_sum(nc_ctx* ctx, const float* x, const int64_t* sig_off, const int64_t* sig_len,
                  const int* group_first, const int64_t* host_len, const int* host_first, int n_groups, float* mid,
                  const int64_t* mid_off, void* stream);
int nc_pv_rotate(nc_ctx* ctx, const float* psi, const float* u_mid, const int64_t* mid_base, const float* u,
                 const int64_t* frame_base, const int* group_first, int n_files, int n_groups, int64_t total_frames,
                 float* phi, void* stream);

/* -------------------------------------------------------------------------
 * MELODIA front end (opt-in; replaces the frame-level part of essentia's
 * PredominantPitchMelodia that pitch.estimate_pitch_melodia calls,
 * pitch.py:210-215: frameSize 2048, hopSize 128).  PARITY UNPINNED: essentia is
 * not installed here; the CPU restatement is oracle/melodia_ref.py.
 *
 * nc_melodia_salience: for every frame t < n_frames[f] of every file f (frame g
 * = frame_base[f] + t; n_frames = ceil((len + 1024) / hop), frames centred at
 * t hop): the 2048-sample frame times win (2048 floats, device: essentia's
 * normalised symmetric Hann), zero-padded to 8192 -> |X| -> the 100 largest
 * spectral peaks (parabolic interpolation) -> the 600-bin, 10-cent pitch
 * salience from 55 Hz (20 harmonics, weight 0.8^h, cos^2 over +-1 semitone,
 * peaks within 40 dB of the frame's largest) -> its local maxima in bins
 * [sal_min_bin, 599], the NC_MELODIA_SALPK largest:
 *   pk_count[g], pk_bin[g * NC_MELODIA_SALPK + i] (int), pk_sal[...] (float),
 *   i < pk_count[g], ordered by salience (descending), ties by bin.
 * frame_base: device int64 [n_files + 1].  No workspace.
 * ------------------------------------------------------------------------- */
#define NC_MELODIA_SALPK 128
int nc_melodia_salience(nc_ctx* ctx, const float* sig, const int64_t* file_off, const int64_t* file_len,
                        const int64_t* frame_base, int n_files, int64_t total_frames, int hop, float sample_rate,
                        const float* win, int sal_min_bin, int* pk_count, int* pk_bin, float* pk_sal,
                        void* stream);
/* nc_melodia_probe (ABI 6; for the tests, not on the product path): the same kernel, the same
 * outputs, and what each stage left, each nullable, device, per frame g:
 *   dbg_mag  [total_frames][4097] float   |X[k]|, k = 0..4096
 *   dbg_npk  [total_frames] int           spectral peaks kept (<= 100)
 *   dbg_pk_f, dbg_pk_a [total_frames][100] double   their frequency (Hz) and magnitude, in the
 *            kernel's order (f32 rounding of the magnitude descending, ties by bin); entries
 *            from dbg_npk[g] on are not written
 *   dbg_sal  [total_frames][600] double   the salience function
 * max_blocks: 0 = the grid of nc_melodia_salience (min(total_frames, 2 x CUs)); > 0 caps it, so
 * that one workgroup walks several frames (results do not depend on it). */
int nc_melodia_probe(nc_ctx* ctx, const float* sig, const int64_t* file_off, const int64_t* file_len,
                     const int64_t* frame_base, int n_files, int64_t total_frames, int hop, float sample_rate,
                     const float* win, int sal_min_bin, int* pk_count, int* pk_bin, float* pk_sal, float* dbg_mag,
                     int* dbg_npk, double* dbg_pk_f, double* dbg_pk_a, double* dbg_sal, int max_blocks,
                     void* stream);

/* -------------------------------------------------------------------------
 * FLAC decode — what the reference gets from librosa.load / soundfile for its FLAC
 * inputs (io.py:44-55).  Native FLAC streams (RFC 9639): 1-8 channels, 4-24 bits per
 * sample, block sizes 1 .. 65535, fixed or variable block size; no Ogg container, no
 * 32-bit samples.  The host walks the container, the device decodes the frames.
 *
 * nc_flac_index (host only, no context; every pointer is HOST memory): skips an ID3v2
 *     tag, requires "fLaC", reads STREAMINFO, skips the other metadata blocks and
 *     lists the frames.  A frame is a header that parses fully (no reserved code,
 *     CRC-8 right, sample size and channel count those of STREAMINFO) and whose frame
 *     or sample number continues the chain from 0, so sync patterns inside a payload
 *     are passed over.
 *       info[8]   = rate, channels, bits per sample, total samples per channel (from
 *                   the frames when STREAMINFO holds 0), min block, max block, byte
 *                   offset of the first frame, 0
 *       md5[16]   = STREAMINFO's MD5 (nullable)
 *       frames    = [cap][8]: byte start, byte end (the next frame's start, or n_bytes),
 *                   first sample, block size, channel assignment (0-7 independent,
 *                   8 left/side, 9 side/right, 10 mid/side), bits per sample, header
 *                   bytes (CRC-8 included), 0 (the file index of a batched decode)
 *       *n_frames = frames found.  cap = 0 (frames may be NULL) only counts.
 *     Status: -1 bad argument, -2 not a stream this decodes (Ogg, no marker, 32-bit or
 *     under 4 bits), -3 cap too small, -4 damaged or truncated (also: the frames do not
 *     add up to STREAMINFO's total).  Reads never leave data[0 .. n_bytes).
 * nc_flac_decode: the frames of several files in one launch, one wave per frame.
 *     data: the files' bytes in one device buffer, 4-byte aligned, data_bytes a
 *     multiple of 4 and at least 8 beyond the last frame's end.  frames: device
 *     int64 [n_frames][8] as above with byte offsets into data and column 7 the file.
 *     files: device int64 [n_files][8] = out_off, channel stride, channels, bits per
 *     sample, total samples, mono_off (-1: no mix), 0, 0.  Channel c of a file is
 *       pcm[out_off + c stride + i]      int32 sample (required; also the work space)
 *       pcm_f32[the same]                sample / 2^(bits-1), exact (nullable)
 *       mono[mono_off + i]               the sample (1 channel) or f32(a + b) 0.5
 *                                        (2 channels); nullable
 *     pcm_len / mono_len: the buffers' lengths in samples; a table row that would
 *     store outside them is refused.  status: device int [n_frames]: 0 ok, 1 CRC-16
 *     mismatch, 2 the bitstream ran past the frame's end, 3 reserved or invalid
 *     field (or table row), 4 decoded length differs from the block size.  A frame
 *     with status 2-4 leaves its samples undefined.  No workspace, no host
 *     synchronisation.
 * ------------------------------------------------------------------------- */
int nc_flac_index(const uint8_t* data, int64_t n_bytes, int64_t* info, uint8_t* md5, int64_t* frames, int64_t cap,
                  int64_t* n_frames);
int nc_flac_decode(nc_ctx* ctx, const uint8_t* data, int64_t data_bytes, const int64_t* frames, int64_t n_frames,
                   const int64_t* files, int n_files, int32_t* pcm, float* pcm_f32, int64_t pcm_len, float* mono,
                   int64_t mono_len, int* status, void* stream);

/* -------------------------------------------------------------------------
 * FLAC encode — what the reference's workflow gets from sox / rubberband / ffmpeg when
 * they write `Song [Nightcore].flac` and its UPD / PS / ADJ versions.  Fixed block size
 * streams, 1-8 channels, 4-24 bits, block 16 .. 16384 (a stream's last frame: 1 .. block);
 * CONSTANT, VERBATIM, FIXED 0-4 and (level 1) LPC 1-8 subframes, Rice partitions of order
 * 0-6 with the exact parameter search, the four stereo assignments; no wasted bits, no
 * escape partitions.  The choice rule is integer-only at level 0 (DESIGN.md §4 "FLAC
 * encode", restated in tests/flac_enc_ref.py); a level 1 frame is never longer than the
 * level 0 frame.  The host writes "fLaC" and STREAMINFO (io.write_flac).
 *
 * nc_flac_encode: the frames of several streams in one launch, one wave per frame.
 *     files:  device int64 [n_files][8] = in_off, channel stride, channels, bits per
 *             sample, sample rate, total samples, 0, 0.  Channel c's sample i is
 *             in[in_off + c stride + i].
 *     frames: device int64 [n_frames][8] = file, first sample, block size, frame number,
 *             slot offset (bytes into slots, a multiple of 4), 0, 0, 0.
 *     Give either pcm_in (int32 samples inside the sample size) or f32_in with pcm_q:
 *     q = clamp(rint(x 2^(bits-1)), -2^(bits-1), 2^(bits-1) - 1), round half to even
 *     (nc_f32_to_pcm16's rule at 16 bits), is stored in pcm_q at the input's index and
 *     clipped[frame] counts the clamped samples.  With pcm_in, pcm_q is nullable and
 *     receives a copy.  in_len: the sample buffers' length.
 *     A frame's slot holds 16 + ceil(channels (8 + block (bits + 1)) / 8) + 2 bytes
 *     rounded up to 4 (all-VERBATIM with the header's bound), which no frame exceeds.
 *     frame_bytes[frame] = the frame's length; records[frame][25] = assignment, then
 *     per channel the subframe type (0 CONSTANT, 1 VERBATIM, 2 FIXED, 3 LPC), order and
 *     partition order; status[frame] = 0 ok, 1 a table row that does not fit the
 *     buffers or the limits above, 2 an int32 sample outside the sample size (nothing
 *     is read or written through such a row; frame_bytes is 0).  No workspace, no host
 *     synchronisation.
 * nc_flac_pack: out[offsets[frame] .. + frame_bytes[frame]) = the frame's slot, for all
 *     frames in one launch; offsets: device int64 [n_frames], the exclusive running sum
 *     of frame_bytes.  out (4-byte aligned, out_bytes a multiple of 4) is zeroed first.
 *     A frame whose row or offset does not fit the buffers is left out.
 * ------------------------------------------------------------------------- */
int nc_flac_encode(nc_ctx* ctx, const int32_t* pcm_in, const float* f32_in, int32_t* pcm_q, int64_t in_len,
                   const int64_t* frames, int64_t n_frames, const int64_t* files, int n_files, int level,
                   uint8_t* slots, int64_t slot_bytes, int* frame_bytes, int* records, int* clipped, int* status,
                   void* stream);
int nc_flac_pack(nc_ctx* ctx, const uint8_t* slots, int64_t slot_bytes, const int64_t* frames, int64_t n_frames,
                 const int* frame_bytes, const int64_t* offsets, uint8_t* out, int64_t out_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NCGPU_H */
