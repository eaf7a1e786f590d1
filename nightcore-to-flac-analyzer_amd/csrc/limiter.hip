// limiter.hip — linked true-peak limiter (what the reference's loudness.apply_true_peak_limiter
// shells out to `ffmpeg -af alimiter=limit=L:attack=5:release=50:level=disabled` for,
// loudness.py:86-134) and the inter-sample peak meter on its own.  PARITY UNPINNED: ffmpeg is
// absent and the reference holds no limiter; the definition is the project's own (DESIGN.md §4
// "True-peak limiter", tests/limiter_ref.py).  For the channels x_c[n], n < N, of one file
// (zero outside), L = 10^(limit_db / 20), Wa / Wr the attack / release in samples, beta = exp(-1 / Wr):
//   h(u) = sinc(u) I0(9 sqrt(1 - (u / 12)^2)) / I0(9), |u| < 12
//   x_c(n + k/4) = sum_{i = -11..12} x_c[n + i] h(k/4 - i), k = 1, 2, 3
//   t[n] = max_c max_k |x_c(n + k/4)|,  p[n] = max(max_c |x_c[n]|, t[n-1], t[n])     (n = -1 included)
//   r[n] = min(1, L / p[n])  (1 where p = 0 and outside the file)
//   hA[n] = min_{0 <= i < Wa} r[n + i],  a[n] = (1 / Wa) sum_{0 <= i < Wa} hA[n - i]
//   d[n] = max(1 - a[n], beta d[n-1]), d[-1] = 0,  g[n] = 1 - d[n]
//   y_c[n] = clamp(x_c[n] g[n], -L, L)
//
// A file is a group of consecutive signals of one length (its channels) in the resident buffer.
// Four launches whatever the lengths, grid.y = file, no host synchronisation, no float atomics
// but the bit-pattern maximum:
//   limiter_peak   8 samples per thread, 2048 per workgroup: the thread loads the 32 samples its
//                  taps reach (16-byte loads; the 12-sample halos overlap its neighbours' in L1,
//                  so no LDS and no barrier), 3 x 24 f32 FMAs per sample and channel, r to the
//                  workspace (f32), the file's true peak by one atomic maximum per workgroup.
//   limiter_gain   one workgroup per 2048-sample tile: its r plus 2 (Wa - 1) halo samples in LDS; the sliding minimum by
//                  log-doubling (floor(log2 Wa) in-place passes, then min(m[i], m[i + Wa - 2^K]));
//                  the box mean from a prefix sum of the deficits 1 - hA in 64-bit fixed point
//                  (units of 2^-45: exact for hA >= 2^-21, order-free, and exactly 0 over a window
//                  of ones, so a = 1 there whatever precedes it); the tile-local max-times scan in
//                  f64 (4 samples per thread, then lanes, then waves); local d (f32) and the tile's
//                  aggregate (f64) to the workspace.  A tile whose span holds no r < 1 leaves early.
//   limiter_carry  one workgroup per file: the tiles' aggregates scanned in tile order (f64),
//                  carry[t] = d at the last sample of tile t - 1.
//   limiter_apply  two tiles per workgroup: d = max(local, beta^(pos + 1) carry), g = (float)(1 - d),
//                  every channel times g and clamped; the output sample peak and
//                  limited[f] = #{n : g[n] < 1}.
// Powers of beta are products of beta^(2^k), k < 22, computed in f64 on the host (closed form,
// no running f32 product), passed by value.
#include <algorithm>
#include <cmath>

#include "nc_device.h"
#include "nc_launch.h"
#include "nc_ws.h"

namespace nc {

constexpr int LM_T = 2048;                               // samples per tile of gain / carry / apply
constexpr int LM_TLOG = 11;
constexpr int LM_WA_MAX = 2048;
constexpr int LM_TAPS = 24;                              // i = -11 .. 12
constexpr int LM_PK_THREADS = 256;
constexpr int LM_PK_SPT = 8;                             // samples per thread of limiter_peak
constexpr int LM_PK_T = LM_PK_THREADS * LM_PK_SPT;       // its tile
constexpr int LM_PK_SPAN = LM_PK_SPT + LM_TAPS;          // x[n - 12 .. n + 20) of a thread
constexpr int LM_PK_WSPAN = 64 * LM_PK_SPT + LM_TAPS;    // ... of a wave (a multiple of 4)
constexpr int LM_THREADS = 512;
constexpr int LM_SPT = LM_T / LM_THREADS;                // 4
constexpr int LM_SPAN = LM_T + 2 * (LM_WA_MAX - 1);      // r span of a tile at the largest attack
constexpr int LM_SPT_SPAN = (LM_SPAN + LM_THREADS - 1) / LM_THREADS;  // 12
constexpr int LM_NE = LM_T + LM_WA_MAX - 1;              // hA values a tile's box means read
constexpr int LM_EPT = (LM_NE + LM_THREADS - 1) / LM_THREADS;         // 8
constexpr int LM_AP_THREADS = 1024;                      // limiter_apply and limiter_carry
constexpr int LM_AP_T = LM_AP_THREADS * LM_SPT;          // two tiles per workgroup of limiter_apply
constexpr int LM_POW = LM_TLOG + 11;                     // beta^(2^k): up to (beta^T)^(2^10)
static_assert(LM_T == 1 << LM_TLOG && LM_SPT == 4 && LM_PK_SPT == 8, "tile layout");

struct LimTaps {
  float c1[LM_TAPS];      // h(1/4 - i) at [i + 11]; h(3/4 - i) is c1[12 - i] (h is even)
  float c2[LM_TAPS / 2];  // h(1/2 - i) at [i + 11], i <= 0; the rest mirrors
};
struct LimPow {
  double p[LM_POW];  // beta^(2^k)
};

// the workspace region of a file of n frames: r[pad] f32, local d[pad] f32, agg[tiles] f64,
// carry[tiles] f64, a multiple of 256 bytes
__host__ __device__ inline int64_t lim_pad(int64_t n) { return (n + 63) / 64 * 64; }
__host__ __device__ inline int64_t lim_tiles(int64_t n) { return (n + LM_T - 1) / LM_T; }
// (LimWs reads on the device what lim_file_carve() lays out on the host)
struct LimWs {
  float* r;
  float* dl;
  double* agg;
  double* carry;
  __device__ LimWs(char* ws, int64_t off, int64_t n) {
    const int64_t pad = lim_pad(n);
    r = reinterpret_cast<float*>(ws + off);
    dl = r + pad;
    agg = reinterpret_cast<double*>(dl + pad);
    carry = agg + lim_tiles(n);
  }
};

static LimTaps make_taps() {
  auto i0 = [](double x) {  // modified Bessel I0 (series)
    double s = 1.0, term = 1.0;
    for (int k = 1; k < 200; ++k) {
      term *= (x / (2.0 * k)) * (x / (2.0 * k));
      s += term;
      if (term < 1e-18 * s) break;
    }
    return s;
  };
  const double den = i0(9.0);
  auto h = [&](double u) {
    const double q = u / 12.0;
    if (!(std::fabs(q) < 1.0)) return 0.0;
    const double sinc = u == 0.0 ? 1.0 : std::sin(M_PI * u) / (M_PI * u);
    return sinc * i0(9.0 * std::sqrt(1.0 - q * q)) / den;
  };
  LimTaps t;
  for (int q = 0; q < LM_TAPS; ++q) t.c1[q] = (float)h(0.25 - (q - 11));
  for (int q = 0; q < LM_TAPS / 2; ++q) t.c2[q] = (float)h(0.5 - (q - 11));
  return t;
}

// prod of pw[k] over the set bits k < NBITS of m: q^m for pw[k] = q^(2^k)
template <int NBITS>
__device__ __forceinline__ double lim_pow_bits(const double* pw, int m) {
  double f = 1.0;
#pragma unroll
  for (int k = 0; k < NBITS; ++k)
    if ((m >> k) & 1) f *= pw[k];
  return f;
}

// Inclusive max-times scan over the workgroup's threads in thread order:
//   out_t = max_{s <= t} q^(t - s) v_s,  pw[k] = q^(2^k), k <= 6;  *excl = out_{t-1} (0 for t = 0).
// red: one double per wave.  All threads call; red is free again on return.
__device__ __forceinline__ double lim_scan(double v, const double* pw, double* red, int tid, double* excl) {
  const int lane = tid & 63, w = tid >> 6;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const double u = __shfl_up(v, 1 << k, 64);
    if (lane >= (1 << k)) v = fmax(v, pw[k] * u);
  }
  if (lane == 63) red[w] = v;
  __syncthreads();
  double c = 0.0;  // the scan at the last thread of the previous wave
  for (int i = 0; i < w; ++i) c = fmax(red[i], pw[6] * c);
  v = fmax(v, lim_pow_bits<7>(pw, lane + 1) * c);
  const double e = __shfl_up(v, 1, 64);
  *excl = lane ? e : c;
  __syncthreads();
  return v;
}

template <bool WRITE_R>
__global__ __launch_bounds__(LM_PK_THREADS) void limiter_peak_kernel(
    const float* __restrict__ x_all, const int64_t* __restrict__ sig_off, const int64_t* __restrict__ sig_len,
    const int* __restrict__ file_first, LimTaps taps, float L, char* ws, const int64_t* __restrict__ ws_off,
    unsigned* true_peak, unsigned long long* span) {
  const Span span_(span);
  __shared__ float red[LM_PK_THREADS / 64];
  __shared__ __attribute__((aligned(16))) float edge[LM_PK_THREADS / 64][LM_PK_WSPAN];
  const int f = blockIdx.y, tid = threadIdx.x;
  const int s0 = file_first[f], C = file_first[f + 1] - s0;
  const int64_t N = sig_len[s0];
  const int64_t n0 = (int64_t)blockIdx.x * LM_PK_T;
  if (n0 >= N) return;
  // the thread's samples n .. n + 7: t[n - 1 + u], u <= 8, reads x[n - 12 .. n + 20), which it
  // loads itself (neighbours overlap in L1: no barrier, every wave on its own)
  const int lane = tid & 63, wv = tid >> 6;
  const int64_t nw = n0 + (int64_t)wv * (64 * LM_PK_SPT);  // the wave's first sample
  const int64_t n = nw + LM_PK_SPT * lane, nb = n - LM_TAPS / 2;
  // the wave's whole span x[nw - 12 .. nw + 512 + 12) lies in the file
  const bool inside = nw >= LM_TAPS / 2 && nw - LM_TAPS / 2 + LM_PK_WSPAN <= N;
  float tm[LM_PK_SPT + 1], am[LM_PK_SPT];  // max over the channels of t[n - 1 ..], |x[n ..]|
#pragma unroll
  for (int u = 0; u <= LM_PK_SPT; ++u) tm[u] = 0.0f;
#pragma unroll
  for (int u = 0; u < LM_PK_SPT; ++u) am[u] = 0.0f;
  for (int c = 0; c < C; ++c) {
    const int64_t xo = sig_off[s0 + c];
    const float* x = x_all + xo;
    float v[LM_PK_SPAN];
    if ((xo & 3) == 0 && inside) {
      // eight 16-byte loads, issued together
      const float4* x4 = reinterpret_cast<const float4*>(x + nb);
#pragma unroll
      for (int q = 0; q < LM_PK_SPAN / 4; ++q) {
        const float4 t4 = x4[q];
        v[4 * q] = t4.x, v[4 * q + 1] = t4.y, v[4 * q + 2] = t4.z, v[4 * q + 3] = t4.w;
      }
    } else {
      // a wave at an end of the file, or a channel off the 16-byte grid: the wave's span through
      // its own LDS row, zero outside the file (a wave's LDS operations complete in order)
      float* e = edge[wv];
      for (int i = lane; i < LM_PK_WSPAN; i += 64) {
        const int64_t m = nw - LM_TAPS / 2 + i;
        e[i] = (m >= 0 && m < N) ? x[m] : 0.0f;
      }
      __builtin_amdgcn_wave_barrier();
      const float4* e4 = reinterpret_cast<const float4*>(e + LM_PK_SPT * lane);
#pragma unroll
      for (int q = 0; q < LM_PK_SPAN / 4; ++q) {
        const float4 t4 = e4[q];
        v[4 * q] = t4.x, v[4 * q + 1] = t4.y, v[4 * q + 2] = t4.z, v[4 * q + 3] = t4.w;
      }
      __builtin_amdgcn_wave_barrier();
    }
#pragma unroll
    for (int u = 0; u <= LM_PK_SPT; ++u) {
      float a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
#pragma unroll
      for (int q = 0; q < LM_TAPS; ++q) {
        a1 = fmaf(v[u + q], taps.c1[q], a1);
        a2 = fmaf(v[u + q], taps.c2[q < LM_TAPS / 2 ? q : LM_TAPS - 1 - q], a2);
        a3 = fmaf(v[u + q], taps.c1[LM_TAPS - 1 - q], a3);
      }
      tm[u] = fmaxf(tm[u], fmaxf(fabsf(a1), fmaxf(fabsf(a2), fabsf(a3))));
    }
#pragma unroll
    for (int u = 0; u < LM_PK_SPT; ++u) am[u] = fmaxf(am[u], fabsf(v[u + LM_TAPS / 2]));
  }
  float r[LM_PK_SPT], pk = 0.0f;
#pragma unroll
  for (int u = 0; u < LM_PK_SPT; ++u) {
    const float p = fmaxf(am[u], fmaxf(tm[u], tm[u + 1]));
    const bool in = n + u < N;
    r[u] = (in && p > 0.0f) ? fminf(1.0f, L / p) : 1.0f;
    pk = in ? fmaxf(pk, p) : pk;
  }
  if (WRITE_R) {
    const LimWs w(ws, ws_off[f], N);
    const int64_t pad = lim_pad(N);
    if (n < pad) *reinterpret_cast<float4*>(w.r + n) = make_float4(r[0], r[1], r[2], r[3]);
    if (n + 4 < pad) *reinterpret_cast<float4*>(w.r + n + 4) = make_float4(r[4], r[5], r[6], r[7]);
  }
  pk = wave_max(pk);
  if ((tid & 63) == 0) red[tid >> 6] = pk;
  __syncthreads();
  if (tid == 0) {
    float m = red[0];
    for (int i = 1; i < LM_PK_THREADS / 64; ++i) m = fmaxf(m, red[i]);
    atomicMax(true_peak + f, __float_as_uint(m));
  }
}

__global__ __launch_bounds__(LM_THREADS) void limiter_gain_kernel(
    const int64_t* __restrict__ sig_len, const int* __restrict__ file_first, int Wa, int K, LimPow bp, char* ws,
    const int64_t* __restrict__ ws_off, unsigned long long* span) {
  const Span span_(span);
  // m (the r span, then its sliding minima) is dead once every thread has formed its deficits,
  // at the barrier before S is written: one 32 KB pool, four workgroups per CU
  __shared__ unsigned long long S[LM_EPT * LM_THREADS];
  static_assert(sizeof(S) >= sizeof(float) * LM_SPT_SPAN * LM_THREADS, "m overlays S");
  float* m = reinterpret_cast<float*>(S);
  __shared__ unsigned long long redu[LM_THREADS / 64];
  __shared__ double red[LM_THREADS / 64];
  const int f = blockIdx.y, tid = threadIdx.x;
  const int64_t N = sig_len[file_first[f]];
  const int64_t n0 = (int64_t)blockIdx.x * LM_T;
  if (n0 >= N) return;
  const LimWs w(ws, ws_off[f], N);
  const int64_t pad = lim_pad(N);
  const int64_t nt = n0 + LM_SPT * tid;  // the thread's four samples
  const int sp = LM_T + 2 * (Wa - 1);    // m[i] = r[n0 - (Wa - 1) + i]
  const int nq = (sp + LM_THREADS - 1) / LM_THREADS;  // passes of the workgroup over the span
  int any = 0;
  {
    float st[LM_SPT_SPAN];  // all loads first (clamped into the file), as in limiter_peak
#pragma unroll
    for (int q = 0; q < LM_SPT_SPAN; ++q) {
      const int64_t n = n0 - (Wa - 1) + tid + q * LM_THREADS;
      st[q] = q < nq ? w.r[min(max(n, (int64_t)0), N - 1)] : 1.0f;
    }
#pragma unroll
    for (int q = 0; q < LM_SPT_SPAN; ++q) {
      const int i = tid + q * LM_THREADS;
      const int64_t n = n0 - (Wa - 1) + i;
      const float v = (n >= 0 && n < N) ? st[q] : 1.0f;
      if (i < sp) {
        m[i] = v;
        any |= v < 1.0f;
      }
    }
  }
  if (!__syncthreads_or(any)) {  // no over-peak within reach of the tile: a = 1, local d = 0
    if (nt < pad) *reinterpret_cast<float4*>(w.dl + nt) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (tid == 0) w.agg[blockIdx.x] = 0.0;
    return;
  }
  // sliding minimum by doubling: after pass k, m[i] = min r[i .. i + 2^(k+1)) for i + 2^(k+1) <= sp
  for (int k = 0; k < K; ++k) {
    const int s = 1 << k;
    float a[LM_SPT_SPAN];
#pragma unroll
    for (int q = 0; q < LM_SPT_SPAN; ++q) {
      const int i = tid + q * LM_THREADS;
      a[q] = (q < nq && i + s < sp) ? fminf(m[i], m[i + s]) : 1.0f;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < LM_SPT_SPAN; ++q) {
      const int i = tid + q * LM_THREADS;
      if (q < nq && i + s < sp) m[i] = a[q];
    }
    __syncthreads();
  }
  // hA[i] = min(m[i], m[i + Wa - 2^K]), i < ne (sample n0 - (Wa - 1) + i); S = inclusive prefix
  // sum of (1 - hA) 2^45 in 64-bit integers
  const int ne = LM_T + Wa - 1, sh = Wa - (1 << K);
  unsigned long long loc[LM_EPT], acc = 0;
#pragma unroll
  for (int q = 0; q < LM_EPT; ++q) {
    const int i = LM_EPT * tid + q;
    if (i < ne) {
      const double e = 1.0 - (double)fminf(m[i], m[i + sh]);
      acc += (unsigned long long)__double2ll_rn(e * 0x1p45);
    }
    loc[q] = acc;
  }
  const int lane = tid & 63, wv = tid >> 6;
  unsigned long long inc = acc;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long u = __shfl_up(inc, o, 64);
    if (lane >= o) inc += u;
  }
  if (lane == 63) redu[wv] = inc;
  __syncthreads();
  unsigned long long base = inc - acc;
  for (int i = 0; i < wv; ++i) base += redu[i];
#pragma unroll
  for (int q = 0; q < LM_EPT; ++q) {
    const int i = LM_EPT * tid + q;
    if (i < ne) S[i] = base + loc[q];
  }
  __syncthreads();
  // 1 - a at the thread's samples j = 4 tid + q: the window hA[j .. j + Wa) of the tile's indexing
  const double scale = 0x1p-45 / (double)Wa;
  const int j = LM_SPT * tid;
  double d[LM_SPT];
#pragma unroll
  for (int q = 0; q < LM_SPT; ++q) {
    const unsigned long long lo = j + q > 0 ? S[j + q - 1] : 0ull;
    d[q] = fmin(1.0, (double)(S[j + q + Wa - 1] - lo) * scale);
  }
  // release: d[n] = max(1 - a[n], beta d[n - 1]) inside the tile (d = 0 before it)
#pragma unroll
  for (int q = 1; q < LM_SPT; ++q) d[q] = fmax(d[q], bp.p[0] * d[q - 1]);
  double c;
  lim_scan(d[LM_SPT - 1], bp.p + 2, red, tid, &c);  // thread step: beta^4
  if (c > 0.0) {
    const double b1 = bp.p[0], b2 = bp.p[1];
    d[0] = fmax(d[0], b1 * c);
    d[1] = fmax(d[1], b2 * c);
    d[2] = fmax(d[2], b1 * b2 * c);
    d[3] = fmax(d[3], bp.p[2] * c);
  }
  if (nt < pad) *reinterpret_cast<float4*>(w.dl + nt) = make_float4((float)d[0], (float)d[1], (float)d[2], (float)d[3]);
  if (tid == LM_THREADS - 1) w.agg[blockIdx.x] = d[LM_SPT - 1];
}

__global__ __launch_bounds__(LM_AP_THREADS) void limiter_carry_kernel(const int64_t* __restrict__ sig_len,
                                                                   const int* __restrict__ file_first, LimPow bp,
                                                                   char* ws, const int64_t* __restrict__ ws_off,
                                                                   unsigned long long* span) {
  const Span span_(span);
  __shared__ double red[LM_AP_THREADS / 64];
  __shared__ double last;
  const int f = blockIdx.x, tid = threadIdx.x;
  const int64_t N = sig_len[file_first[f]];
  const int64_t nt = lim_tiles(N);
  if (nt == 0) return;
  const LimWs w(ws, ws_off[f], N);
  const double* pw = bp.p + LM_TLOG;  // tile step: beta^T
  double R = 0.0;                     // d at the last sample before this chunk of tiles
  for (int64_t b = 0; b < nt; b += LM_AP_THREADS) {
    const int64_t t = b + tid;
    double ex;
    double v = lim_scan(t < nt ? w.agg[t] : 0.0, pw, red, tid, &ex);
    if (R > 0.0) v = fmax(v, lim_pow_bits<11>(pw, tid + 1) * R);
    if (t + 1 < nt) w.carry[t + 1] = v;
    if (tid == LM_AP_THREADS - 1) last = v;
    __syncthreads();
    R = last;
    __syncthreads();
  }
  if (tid == 0) w.carry[0] = 0.0;
}

// x and y may be the same buffer (in place): a thread reads and writes its own samples only
__global__ __launch_bounds__(LM_AP_THREADS) void limiter_apply_kernel(
    const float* x_all, const int64_t* __restrict__ sig_off, const int64_t* __restrict__ sig_len,
    const int* __restrict__ file_first, float* y_all, const int64_t* __restrict__ y_off, LimPow bp, float L, char* ws,
    const int64_t* __restrict__ ws_off, unsigned* peak_out, int* limited, unsigned long long* span) {
  const Span span_(span);
  __shared__ float red[LM_AP_THREADS / 64];
  __shared__ int redc[LM_AP_THREADS / 64];
  const int f = blockIdx.y, tid = threadIdx.x;
  const int s0 = file_first[f], C = file_first[f + 1] - s0;
  const int64_t N = sig_len[s0];
  const int64_t n0 = (int64_t)blockIdx.x * LM_AP_T;
  if (n0 >= N) return;
  const LimWs w(ws, ws_off[f], N);
  const int64_t n = n0 + LM_SPT * tid;
  const int j = (int)(n & (LM_T - 1));  // position in the tile (a wave's 256 samples share one tile)
  const double carry = n < N ? w.carry[n >> LM_TLOG] : 0.0;
  double d[LM_SPT] = {0.0, 0.0, 0.0, 0.0};
  if (n < N) {  // n < pad and the four of them inside r's padding
    const float4 l4 = *reinterpret_cast<const float4*>(w.dl + n);
    d[0] = l4.x, d[1] = l4.y, d[2] = l4.z, d[3] = l4.w;
  }
  if (carry > 0.0) {
    double fct = lim_pow_bits<LM_TLOG + 1>(bp.p, j + 1) * carry;  // beta^(pos + 1) carry
#pragma unroll
    for (int q = 0; q < LM_SPT; ++q) {
      d[q] = fmax(d[q], fct);
      fct *= bp.p[0];
    }
  }
  float g[LM_SPT];
  int cnt = 0;
#pragma unroll
  for (int q = 0; q < LM_SPT; ++q) {
    g[q] = (float)(1.0 - d[q]);
    cnt += (n + q < N && g[q] < 1.0f) ? 1 : 0;
  }
  float pk = 0.0f;
  for (int c = 0; c < C; ++c) {
    const int64_t xo = sig_off[s0 + c], yo = y_off[s0 + c];
    const float* x = x_all + xo + n;
    float* y = y_all + yo + n;
    if (n + LM_SPT <= N && ((xo | yo) & 3) == 0) {
      const float4 x4 = *reinterpret_cast<const float4*>(x);
      float4 y4;
      y4.x = fminf(fmaxf(x4.x * g[0], -L), L);
      y4.y = fminf(fmaxf(x4.y * g[1], -L), L);
      y4.z = fminf(fmaxf(x4.z * g[2], -L), L);
      y4.w = fminf(fmaxf(x4.w * g[3], -L), L);
      *reinterpret_cast<float4*>(y) = y4;
      pk = fmaxf(pk, fmaxf(fmaxf(fabsf(y4.x), fabsf(y4.y)), fmaxf(fabsf(y4.z), fabsf(y4.w))));
    } else {
#pragma unroll
      for (int q = 0; q < LM_SPT; ++q)
        if (n + q < N) {
          const float v = fminf(fmaxf(x[q] * g[q], -L), L);
          y[q] = v;
          pk = fmaxf(pk, fabsf(v));
        }
    }
  }
  pk = wave_max(pk);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  if ((tid & 63) == 0) red[tid >> 6] = pk, redc[tid >> 6] = cnt;
  __syncthreads();
  if (tid == 0) {
    float mx = red[0];
    int tot = redc[0];
    for (int i = 1; i < LM_AP_THREADS / 64; ++i) mx = fmaxf(mx, red[i]), tot += redc[i];
    atomicMax(peak_out + f, __float_as_uint(mx));
    if (tot) atomicAdd(limited + f, tot);
  }
}

// the region of a file of n frames, appended to the files before it; returns its offset
static size_t lim_file_carve(WsCarve& c, int64_t n) {
  const size_t off = c.bytes(), pad = (size_t)lim_pad(n), tiles = (size_t)lim_tiles(n);
  c.skip(pad * sizeof(float), 4);     // r
  c.skip(pad * sizeof(float), 4);     // local d
  c.skip(tiles * sizeof(double), 8);  // agg
  c.skip(tiles * sizeof(double), 8);  // carry
  c.skip(0);
  return off;
}

// nc_limiter_ws_bytes: the files' regions back to back
size_t limiter_ws_bytes(const int64_t* n_frames, int n_files, int64_t* ws_off) {
  WsCarve c;
  for (int f = 0; f < n_files; ++f) {
    const size_t off = lim_file_carve(c, std::max<int64_t>(0, n_frames[f]));
    if (ws_off) ws_off[f] = (int64_t)off;
  }
  return c.bytes();
}

// the groups of one call, from the host's copy of the descriptors
static int lim_check(const char* who, const int64_t* host_len, const int* host_first, int n_files, int64_t* max_len,
                     size_t* ws_need) {
  const std::string w(who);
  if (n_files > 65535) {
    set_error(w + ": at most 65535 files in one call");
    return -2;
  }
  if (!host_len || !host_first || host_first[0] != 0) {
    set_error(w + ": host_len and host_first (starting at 0) are required");
    return -2;
  }
  *max_len = 0;
  WsCarve c;
  for (int f = 0; f < n_files; ++f) {
    const int s0 = host_first[f], C = host_first[f + 1] - s0;
    if (C < 1) {
      set_error(w + ": every file needs at least one channel");
      return -2;
    }
    const int64_t n = host_len[s0];
    if (n < 0 || n > (INT64_C(1) << 40)) {
      set_error(w + ": length outside 0 .. 2^40");
      return -2;
    }
    for (int c = 1; c < C; ++c)
      if (host_len[s0 + c] != n) {
        set_error(w + ": the channels of a file must be equally long");
        return -2;
      }
    *max_len = std::max(*max_len, n);
    lim_file_carve(c, n);
  }
  *ws_need = c.bytes();
  return 0;
}

int launch_true_peak(Context& ctx, const float* x, const int64_t* sig_off, const int64_t* sig_len,
                     const int* file_first, const int64_t* host_len, const int* host_first, int n_files,
                     float* true_peak, hipStream_t st) {
  if (n_files <= 0) return 0;
  int64_t max_len;
  size_t need;
  if (int rc = lim_check("true_peak", host_len, host_first, n_files, &max_len, &need)) return rc;
  NC_HIP(hipMemsetAsync(true_peak, 0, (size_t)n_files * sizeof(float), st));
  if (max_len <= 0) return 0;
  static const LimTaps taps = make_taps();
  {
    KTimer kt_(ctx, "limiter_peak", st);
    hipLaunchKernelGGL(limiter_peak_kernel<false>, dim3((unsigned)((max_len + LM_PK_T - 1) / LM_PK_T), (unsigned)n_files),
                       dim3(LM_PK_THREADS), 0, st, x, sig_off, sig_len, file_first, taps, 1.0f, (char*)nullptr,
                       (const int64_t*)nullptr, reinterpret_cast<unsigned*>(true_peak), kt_.span());
  }
  NC_HIP(hipGetLastError());
  return 0;
}

int launch_true_peak_limit(Context& ctx, const float* x, const int64_t* sig_off, const int64_t* sig_len,
                           const int* file_first, const int64_t* host_len, const int* host_first, int n_files,
                           double limit_db, int attack, int release, float* y, const int64_t* y_off,
                           float* true_peak, float* peak_out, int* limited, void* ws, const int64_t* ws_off,
                           size_t ws_bytes, hipStream_t st) {
  if (n_files <= 0) return 0;
  if (!(limit_db <= 0.0) || !std::isfinite(limit_db)) {
    set_error("true_peak_limit: the ceiling must be at or below 0 dBFS");
    return -2;
  }
  if (attack < 1 || attack > LM_WA_MAX || release < 1) {
    set_error("true_peak_limit: attack outside 1 .. 2048 samples, or release below 1 sample");
    return -2;
  }
  int64_t max_len;
  size_t need;
  if (int rc = lim_check("true_peak_limit", host_len, host_first, n_files, &max_len, &need)) return rc;
  if (need > ws_bytes || (need > 0 && (!ws || !ws_off))) {
    set_error("true_peak_limit: workspace smaller than nc_limiter_ws_bytes");
    return -2;
  }
  NC_HIP(hipMemsetAsync(true_peak, 0, (size_t)n_files * sizeof(float), st));
  NC_HIP(hipMemsetAsync(peak_out, 0, (size_t)n_files * sizeof(float), st));
  NC_HIP(hipMemsetAsync(limited, 0, (size_t)n_files * sizeof(int), st));
  if (max_len <= 0) return 0;
  static const LimTaps taps = make_taps();
  LimPow bp;
  for (int k = 0; k < LM_POW; ++k) bp.p[k] = std::exp(-std::ldexp(1.0, k) / (double)release);
  const float L = (float)std::pow(10.0, limit_db / 20.0);
  int K = 0;
  while ((2 << K) <= attack) ++K;  // floor(log2(attack))
  const dim3 grid((unsigned)lim_tiles(max_len), (unsigned)n_files);
  char* wsb = static_cast<char*>(ws);
  {
    KTimer kt_(ctx, "limiter_peak", st);
    hipLaunchKernelGGL(limiter_peak_kernel<true>, dim3((unsigned)((max_len + LM_PK_T - 1) / LM_PK_T), grid.y),
                       dim3(LM_PK_THREADS), 0, st, x, sig_off, sig_len, file_first,
                       taps, L, wsb, ws_off, reinterpret_cast<unsigned*>(true_peak), kt_.span());
  }
  {
    KTimer kt_(ctx, "limiter_gain", st);
    hipLaunchKernelGGL(limiter_gain_kernel, grid, dim3(LM_THREADS), 0, st, sig_len, file_first, attack, K, bp, wsb,
                       ws_off, kt_.span());
  }
  {
    KTimer kt_(ctx, "limiter_carry", st);
    hipLaunchKernelGGL(limiter_carry_kernel, dim3((unsigned)n_files), dim3(LM_AP_THREADS), 0, st, sig_len, file_first,
                       bp, wsb, ws_off, kt_.span());
  }
  {
    KTimer kt_(ctx, "limiter_apply", st);
    hipLaunchKernelGGL(limiter_apply_kernel, dim3((unsigned)((max_len + LM_AP_T - 1) / LM_AP_T), grid.y),
                       dim3(LM_AP_THREADS), 0, st, x, sig_off, sig_len, file_first, y, y_off,
                       bp, L, wsb, ws_off, reinterpret_cast<unsigned*>(peak_out), limited, kt_.span());
  }
  NC_HIP(hipGetLastError());
  return 0;
}

}  // namespace nc
