// nc_launch.h — the launchers, size queries and plans that the .hip translation units define
// and nc_capi.cpp calls.  Both sides include this header, so a drifted prototype fails to
// compile where it is defined instead of at link time.
#pragma once
#include "nc_engine.h"

namespace nc {

int launch_melodia_salience(Context& ctx, const float* sig, const int64_t* file_off, const int64_t* file_len,
                            const int64_t* frame_base, int n_files, int64_t total_frames, int hop, float sr,
                            const float* win, int sal_min_bin, int* pk_count, int* pk_bin, float* pk_sal,
                            float* dbg_mag, int* dbg_npk, double* dbg_pk_f, double* dbg_pk_a, double* dbg_sal,
                            int max_blocks, hipStream_t st);
size_t window_stage_ws_bytes(const Context& ctx, int n_win, int T);
int launch_window_stage(Context& ctx, const float* sig, const int64_t* win_off, const uint8_t* active,
                        int n_win, int win_len, int hop, float* onset_out, double* tg_out,
                        double* energy_out, const int* win_chunk, const int64_t* chunk_tf_base, int tp_frames,
                        float* peak_pitch, float* peak_mag, int* chunk_npk, void* stft_done,
                        void* ws, size_t ws_bytes, hipStream_t st);
size_t tempo_beats_ws_bytes(int64_t total_frames);
int launch_tempo_beats_c(Context& ctx, const float* onset, const int64_t* off, const int* len, int n_seq,
                         int max_len, const double* tg, int acw, const double* start_bpm,
                         const int* prior_idx, const uint8_t* active, int hop, int trim, double* bpm_out,
                         int* lag_out, int* nbeats_out, double* margin_out, int* beats_out,
                         int64_t total_frames, void* ws, size_t ws_bytes, hipStream_t st);
int launch_nc_prior(const double* bpm, const int* nbeats, const uint8_t* active, const int* src_w0,
                    const int* src_w1, const int64_t* src_len, const int64_t* nc_len, int n_pairs,
                    double* prior_out, hipStream_t st, int sr);
int launch_ibi_from_beats(const int* beats, const int64_t* off, const int* nbeats, int n_seq, int hop,
                          int min_ibis, double* ibi_out, int* n_ibi, hipStream_t st, int sr);
size_t trim_ws_bytes(const int64_t* host_file_len, int n_files);
int launch_trim(Context& ctx, const float* sig, const int64_t* file_off, const int64_t* file_len, int n_files,
                int64_t max_frames, float top_db, int64_t* out_start, int64_t* out_end, void* ws,
                size_t ws_bytes, hipStream_t st);

size_t chroma_ws_bytes(int n, int64_t total_len);
int chroma_ws_layout_query(int n, int64_t total_len, int64_t* out, int cap);
int launch_chroma_mean(Context& ctx, const float* sig, const int64_t* chunk_off, const int64_t* chunk_len, int n,
                       int64_t total_len, int64_t max_chunk_len, float* out_chroma, float* out_tuning,
                       int* out_tuning_idx, int* out_tuning_margin, const int* tf_skip, int64_t tf_skip_total,
                       float* ext_pitch,
                       float* ext_mag, int* ext_npk, void* wait_event, void* ws, size_t ws_bytes, hipStream_t st);
int launch_chroma_lag(const float* chroma, const int* src_idx, const int* nc_idx, int n_pairs, int* lag_out,
                      double* margin_out, hipStream_t st);
int launch_xcorr_peak(const float* a, const float* b, int n, int n_pairs, int* lag_out, hipStream_t st);

size_t bootstrap_job_bytes(int cap, int n_boot);
int launch_bootstrap(const BootArgs& a, int n_jobs, hipStream_t st);

size_t ibi_onset_ws_bytes(int n_files, int64_t total_frames);
int launch_ibi_onset(Context& ctx, const float* sig, const int64_t* file_off, const int64_t* file_len, int n_files,
                     int64_t total_frames, int hop, float* onset_out, int64_t* frame_base_out, void* ws,
                     size_t ws_bytes, hipStream_t st);
size_t ibi_tg_ws_bytes(const Context& ctx, int n_files, int64_t total_frames, int max_frames, int hop);
int launch_ibi_tempogram(Context& ctx, const float* onset, const int64_t* frame_base, int n_files,
                         int64_t total_frames, int max_frames, int hop,
                         double* tg_out, void* ws, size_t ws_bytes, hipStream_t st);

size_t ibi_range_ws_bytes(int n_files, int64_t total_rows);
int launch_ibi_mel_range(Context& ctx, const float* sig, const int64_t* file_off, const int64_t* file_len,
                         int n_files, const int64_t* t0, const int64_t* t1, int hop, int64_t total_rows,
                         float* max_out, void* ws, size_t ws_bytes, hipStream_t st);
int launch_ibi_onset_range(int n_files, const int64_t* t0, int hop, int64_t total_out, const float* gmax,
                           float* onset_out, void* ws, int64_t total_rows, hipStream_t st);
int launch_ibi_tempogram_tiles(Context& ctx, const float* onset, const int64_t* frame_base, int n_files,
                               int64_t total_frames, int max_frames, int hop, const int64_t* b0, const int64_t* b1,
                               double* slab_out, double* tg_out, void* ws, size_t ws_bytes, hipStream_t st);
int launch_ibi_tempogram_reduce(Context& ctx, const double* slab, const int64_t* frame_base, int n_files,
                                int max_frames, int hop, double* tg_out, hipStream_t st);

size_t align_ws_bytes(int n_pairs, int n_speeds, int64_t total_len, int64_t max_len, int max_off_frames);
int launch_align_offsets(Context& ctx, const float* sig, const int64_t* src_off, const int64_t* src_len,
                         const int64_t* nc_off, const int64_t* nc_len, int n_pairs, const double* speeds,
                         int n_speeds, int max_off_frames, int64_t total_len, int64_t max_len, int* out_peak,
                         int* out_speed, double* out_score, void* ws, size_t ws_bytes, hipStream_t st);
int launch_xcorr(const float* sig, const int64_t* ia, const int64_t* ib, int n_items, int win, double* dot,
                 double* sqb, const int* w0, const int* w1, const int* sw, const int* c0, const int* c1,
                 const int64_t* pa, const int64_t* pbv, const int64_t* exp_pb, int n_jobs, double* ratio_out,
                 double* quality_out, hipStream_t st);

size_t spectral_ws_bytes(int64_t total_frames, int n_files, int64_t max_frames);
int launch_spectral(Context& ctx, const float* sig, const int64_t* file_off, const int64_t* file_len,
                    const int64_t* frame_base, const double* bin_hz, const int* band_bins, int n_files,
                    int64_t total_frames, int64_t max_frames, float roll_percent, float* rms_out,
                    double* stats_out, double* bin_db_out, void* ws, size_t ws_bytes, hipStream_t st);

int launch_pcm16_to_f32(const int16_t* x, int64_t n, float* y, hipStream_t st);
int launch_window_energy_blocks(const float* sig, const void* trim_ws, int n_files, const int64_t* file_off,
                                const int64_t* win_off, const int* win_file, int n_win, int win_len, double* out,
                                hipStream_t st);
int launch_resample_poly(const float* x, const int64_t* in_off, const int64_t* in_len, int n_files,
                         float* y, const int64_t* out_off, const int64_t* out_len, int64_t max_out,
                         const double* h, int h_len, int up, int down, int64_t pre_remove, hipStream_t st);

int64_t speed_factor_p(double factor);
int64_t speed_out_len_host(int64_t n, int64_t P);
int launch_speed_render(Context& ctx, const float* x, const int64_t* in_off, const int64_t* in_len, int n_files,
                        int64_t P, float* y, const int64_t* out_off, int64_t max_out, float* peak, hipStream_t st);
int launch_f32_to_pcm16(const float* x, const int64_t* in_off, const int64_t* in_len, int n_files, int64_t max_len,
                        int16_t* q, const int64_t* out_off, int64_t out_stride, int* clipped, hipStream_t st);

size_t limiter_ws_bytes(const int64_t* n_frames, int n_files, int64_t* ws_off);
int launch_true_peak(Context& ctx, const float* x, const int64_t* sig_off, const int64_t* sig_len,
                     const int* file_first, const int64_t* host_len, const int* host_first, int n_files,
                     float* true_peak, hipStream_t st);
int launch_true_peak_limit(Context& ctx, const float* x, const int64_t* sig_off, const int64_t* sig_len,
                           const int* file_first, const int64_t* host_len, const int* host_first, int n_files,
                           double limit_db, int attack, int release, float* y, const int64_t* y_off,
                           float* true_peak, float* peak_out, int* limited, void* ws, const int64_t* ws_off,
                           size_t ws_bytes, hipStream_t st);

int pv_plan(int64_t P, const int64_t* n_in, int n_files, int64_t* ns_out, int64_t* k_out, int64_t* frame_base,
            int64_t* ws_off, size_t* ws_bytes);
size_t pv_scan_ws_bytes(int64_t total_frames, int n_files);
int launch_pv_analyze(Context& ctx, const float* x, const int64_t* in_off, const int64_t* in_len,
                      const int64_t* frame_base, int n_files, int64_t total_frames, int64_t P, float* mag, float2* V,
                      uint8_t* empty, float2* U, bool with_u, hipStream_t st);
size_t pv_lock_ws_bytes(int64_t total_frames, int n_files);
int launch_pv_lock(Context& ctx, const float* mag, const float2* U, const float2* V, const uint8_t* empty,
                   const int64_t* frame_base, int n_files, int64_t total_frames, int64_t max_frames, float2* phi,
                   uint16_t* owner, void* ws, size_t ws_bytes, hipStream_t st);
int launch_pv_mid_sum(Context& ctx, const float* x, const int64_t* sig_off, const int64_t* sig_len,
                      const int* group_first, const int64_t* host_len, const int* host_first, int n_groups,
                      float* mid, const int64_t* mid_off, hipStream_t st);
int launch_pv_rotate(Context& ctx, const float2* psi, const float2* u_mid, const int64_t* mid_base, const float2* u,
                     const int64_t* frame_base, const int* group_first, int n_files, int n_groups,
                     int64_t total_frames, float2* phi, hipStream_t st);
int launch_pv_scan(Context& ctx, const float2* V, const uint8_t* empty, const int64_t* frame_base, int n_files,
                   int64_t total_frames, int64_t max_frames, float2* phi, void* ws, size_t ws_bytes, hipStream_t st);
int launch_pv_synth(Context& ctx, const float* mag, const float2* phi, const int64_t* in_len,
                    const int64_t* frame_base, int n_files, int64_t total_frames, int64_t P, int64_t max_ns,
                    float* frames, size_t frames_bytes, float* s, const int64_t* out_off, float* peak,
                    hipStream_t st);
int launch_pv_stretch(Context& ctx, const float* x, const int64_t* in_off, const int64_t* in_len,
                      const int64_t* frame_base, int n_files, int64_t total_frames, int64_t max_frames, int64_t P,
                      int64_t max_ns, float* s, const int64_t* out_off, float* peak, void* ws, const int64_t* ws_off,
                      size_t ws_bytes, hipStream_t st);

int launch_energy_gate(const double* energy, const int* w0, const int* w1, int n_groups, double gate_db,
                       uint8_t* active, hipStream_t st);
int launch_collect_valid(const double* bpm, const int* nbeats, const uint8_t* active, const int* w0, const int* w1,
                         int n_groups, int min_beats, double* out_values, int* out_n, hipStream_t st);
int launch_pitch_hz(const int* lags, int n, double* shift_out, double* nc_hz, double* src_hz, hipStream_t st);
int launch_window_energy(const float* sig, const int64_t* off, int n, int win_len, double* out, hipStream_t st);
int launch_flac_decode(const uint8_t* data, int64_t data_bytes, const int64_t* frames, int64_t n_frames,
                       const int64_t* files, int n_files, int* pcm, float* f32, int64_t pcm_len, float* mono,
                       int64_t mono_len, int* status, hipStream_t st);
int launch_flac_encode(const int* pcm_in, const float* f32_in, int* pcm_q, int64_t in_len, const int64_t* frames,
                       int64_t n_frames, const int64_t* files, int n_files, int level, uint8_t* slots,
                       int64_t slot_bytes, int* frame_bytes, int* records, int* clipped, int* status, hipStream_t st);
int launch_flac_pack(const uint8_t* slots, int64_t slot_bytes, const int64_t* frames, int64_t n_frames,
                     const int* frame_bytes, const int64_t* offsets, uint8_t* out, int64_t out_bytes, hipStream_t st);

}  // namespace nc
