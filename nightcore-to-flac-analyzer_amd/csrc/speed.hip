// speed.hip — arbitrary-ratio band-limited speed renderer (what the reference's workflow
// shells out to `sox … speed F` for, workflow.py:108-118) and the f32 -> 16-bit PCM epilogue
// of the WAV writer.  PARITY UNPINNED: sox is absent and the reference holds no resampler;
// the definition is the project's own (tests/speed_ref.py):
//   Q = 1e6, Z = 32, BETA = 10.06, ROLL = 0.9;  P = round(F Q) (the six decimals the reference
//   hands to sox), n_out = ceil(n Q / P), c = ROLL min(1, Q / P),
//   t_m = (m P div Q) + ((m P mod Q) / Q)                        exact in int64,
//   h(u) = c g(c u),  g(v) = sinc(v) I0(BETA sqrt(1 - (v / Z)^2)) / I0(BETA) for |v| < Z, else 0,
//   y[m] = sum_j x[j] h(t_m - j)                                 x zero outside [0, n).
// No case is special (F = 1 runs the same path).
//
// MI355X layout: one workgroup of 1024 threads renders SP_OUT = 2048 consecutive outputs of one
// file (grid.y = file; the channels of a stereo file are two files).  It stages g on the grid
// v = i / 512, i <= 32 * 512 (Tables::speed_tab, 64 KB f32) and its own input span
// ((SP_OUT - 1) P / Q + 2 H + 2 samples, H = ceil(Z / c) <= 143: at most 8478 floats) through
// LDS once: ~100 KB of the CU's 160 KB, one workgroup = 16 waves per CU.  Each thread then
// walks the 2 H + 2 taps of its output: the tap's table position |H - q + fr| c 512 in f32,
// g by linear interpolation, one f32 FMA chain in tap order (deterministic).  The position
// m P is int64 (it passes 2^40 within 20 s of 44.1 kHz audio); everything inside the tile is 32-bit.
// peak[f] = max_m |y[m]| comes from the same launch (wave and workgroup maximum, then one
// atomic maximum per workgroup on the bit pattern of the non-negative float: order-free).
#include <algorithm>
#include <cmath>

#include "nc_device.h"
#include "nc_launch.h"

namespace nc {

constexpr int64_t SP_Q = 1000000;
constexpr int SP_Z = 32;
constexpr int SP_TPZ = 512;                  // table points per zero crossing
constexpr int SP_TAB = SP_Z * SP_TPZ + 1;    // g(0) .. g(Z)
constexpr int SP_THREADS = 1024;
constexpr int SP_OPT = 2;                    // outputs per thread
constexpr int SP_OUT = SP_THREADS * SP_OPT;  // outputs per workgroup
constexpr int SP_HMAX = 143;                 // ceil(Z / c) at F = 4
constexpr int SP_TILE = (SP_OUT - 1) * 4 + 2 * SP_HMAX + 2 + 30;  // 8508: input span at F = 4, padded

__host__ __device__ inline int64_t speed_out_len(int64_t n, int64_t P) { return n <= 0 ? 0 : (n * SP_Q + P - 1) / P; }

// P = round(F Q) (half to even, as Python's round) or -1 outside [0.25, 4]
int64_t speed_factor_p(double factor) {
  if (!(factor >= 0.25 && factor <= 4.0)) return -1;
  const int64_t P = (int64_t)std::nearbyint(factor * (double)SP_Q);
  return (P < SP_Q / 4 || P > 4 * SP_Q) ? -1 : P;
}

int64_t speed_out_len_host(int64_t n, int64_t P) { return speed_out_len(n, P); }

// g on the grid i / SP_TPZ in f64, rounded to f32 (build_tables)
void speed_table(float* tab) {
  const double beta = 10.06;
  auto i0 = [](double x) {  // modified Bessel I0 (series)
    double s = 1.0, term = 1.0;
    for (int k = 1; k < 200; ++k) {
      term *= (x / (2.0 * k)) * (x / (2.0 * k));
      s += term;
      if (term < 1e-18 * s) break;
    }
    return s;
  };
  const double den = i0(beta);
  for (int i = 0; i < SP_TAB; ++i) {
    const double v = (double)i / SP_TPZ, r = v / SP_Z;
    const double sinc = i == 0 ? 1.0 : std::sin(M_PI * v) / (M_PI * v);
    tab[i] = (float)(sinc * i0(beta * std::sqrt(std::max(0.0, 1.0 - r * r))) / den);
  }
}
int speed_table_len() { return SP_TAB; }

__global__ __launch_bounds__(SP_THREADS) void speed_render_kernel(
    const float* __restrict__ x_all, const int64_t* __restrict__ in_off, const int64_t* __restrict__ in_len,
    float* __restrict__ y_all, const int64_t* __restrict__ out_off, const float* __restrict__ tab_g, int64_t P, int H,
    float S, float c, unsigned* peak, unsigned long long* span) {
  const Span span_(span);
  __shared__ float tab[SP_TAB + 3];
  __shared__ float tile[SP_TILE];
  __shared__ float red[SP_THREADS / 64];
  const int f = blockIdx.y;
  const int tid = threadIdx.x;
  const int64_t n = in_len[f];
  const int64_t n_out = speed_out_len(n, P);
  const int64_t m0 = (int64_t)blockIdx.x * SP_OUT;
  if (m0 >= n_out) return;
  const int64_t m1 = min(n_out, m0 + SP_OUT);
  // input span of the workgroup: taps i0 - H .. i0 + H + 1 of its first and last output
  const int64_t first = m0 * P / SP_Q - H;
  const int64_t last = (m1 - 1) * P / SP_Q + H + 1;
  const int len = (int)min(last - first + 1, (int64_t)SP_TILE);  // <= SP_TILE for P <= 4 Q (checked by the host)
  for (int i = tid; i < SP_TAB; i += SP_THREADS) tab[i] = tab_g[i];
  const float* x = x_all + in_off[f];
  for (int i = tid; i < len; i += SP_THREADS) {
    const int64_t xi = first + i;
    tile[i] = (xi >= 0 && xi < n) ? x[xi] : 0.0f;
  }
  __syncthreads();

  const int K = 2 * H + 2;
  const float p_end = (float)(SP_Z * SP_TPZ);
  float* y = y_all + out_off[f];
  float pk = 0.0f;
#pragma unroll
  for (int o = 0; o < SP_OPT; ++o) {
    const int64_t m = m0 + o * SP_THREADS + tid;
    if (m < m1) {
      const int64_t pos = m * P;
      const int64_t i0 = pos / SP_Q;
      const float fr = (float)((double)(int)(pos - i0 * SP_Q) / (double)SP_Q);
      const int b = min(max((int)(i0 - H - first), 0), SP_TILE - K);  // in range by construction; clamped anyway
      const float* tb = tile + b;
      float acc = 0.0f;
#pragma unroll 4
      for (int q = 0; q < K; ++q) {
        const float p = fabsf((float)(H - q) + fr) * S;      // |t_m - j| c SP_TPZ
        const int idx = min((int)p, SP_TAB - 2);
        const float w = p - (float)idx;
        const float g0 = tab[idx], g1 = tab[idx + 1];
        const float g = p < p_end ? fmaf(w, g1 - g0, g0) : 0.0f;
        acc = fmaf(tb[q], g, acc);
      }
      const float v = c * acc;
      y[m] = v;
      pk = fmaxf(pk, fabsf(v));
    }
  }
  // per-file peak: wave maximum, workgroup maximum, one atomic per workgroup
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) pk = fmaxf(pk, __shfl_xor(pk, d, 64));
  if ((tid & 63) == 0) red[tid >> 6] = pk;
  __syncthreads();
  if (tid == 0) {
    float v = red[0];
    for (int w = 1; w < SP_THREADS / 64; ++w) v = fmaxf(v, red[w]);
    atomicMax(peak + f, __float_as_uint(v));
  }
}

int launch_speed_render(Context& ctx, const float* x, const int64_t* in_off, const int64_t* in_len, int n_files,
                        int64_t P, float* y, const int64_t* out_off, int64_t max_out, float* peak, hipStream_t st) {
  if (n_files <= 0) return 0;
  if (P < SP_Q / 4 || P > 4 * SP_Q) {
    set_error("speed_render: factor outside [0.25, 4] (P = round(F 1e6))");
    return -2;
  }
  if (!ctx.t.speed_tab) {
    set_error("speed_render: filter table missing");
    return -1;
  }
  if (n_files > 65535 || max_out > (int64_t)SP_OUT * 0x7fffffff) {
    set_error("speed_render: too many files or outputs for one launch");
    return -2;
  }
  NC_HIP(hipMemsetAsync(peak, 0, (size_t)n_files * sizeof(float), st));
  if (max_out <= 0) return 0;
  const int H = (int)((320 * std::max(P, SP_Q) + 9 * SP_Q - 1) / (9 * SP_Q));  // ceil(Z / c)
  const double c = 0.9 * std::min(1.0, (double)SP_Q / (double)P);
  const dim3 grid((unsigned)((max_out + SP_OUT - 1) / SP_OUT), (unsigned)n_files);
  {
    KTimer kt_(ctx, "speed_render", st);
    hipLaunchKernelGGL(speed_render_kernel, grid, dim3(SP_THREADS), 0, st, x, in_off, in_len, y, out_off,
                       ctx.t.speed_tab, P, H, (float)(c * SP_TPZ), (float)c, reinterpret_cast<unsigned*>(peak),
                       kt_.span());
  }
  NC_HIP(hipGetLastError());
  return 0;
}

// f32 -> 16-bit PCM (the mirror of pcm16_to_f32_kernel; io.write_wav of a PCM16 file):
//   q = clamp(rint(x 32768), -32768, 32767), round half to even (x 32768 is exact in f32),
// file f's sample i to q[out_off[f] + i out_stride] (out_stride = channels interleaves the
// channels of one WAV file), clipped[f] = samples whose rounded value fell outside the range.
__global__ __launch_bounds__(256) void f32_to_pcm16_kernel(const float* __restrict__ x_all,
                                                           const int64_t* __restrict__ in_off,
                                                           const int64_t* __restrict__ in_len, int16_t* __restrict__ q_all,
                                                           const int64_t* __restrict__ out_off, int64_t out_stride,
                                                           int* clipped) {
  const int f = blockIdx.y;
  const int64_t n = in_len[f];
  const float* x = x_all + in_off[f];
  int16_t* q = q_all + out_off[f];
  int cnt = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float v = rintf(x[i] * 32768.0f);
    cnt += (v > 32767.0f || v < -32768.0f) ? 1 : 0;
    q[i * out_stride] = (int16_t)(int)fminf(fmaxf(v, -32768.0f), 32767.0f);
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) cnt += __shfl_xor(cnt, d, 64);
  if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(clipped + f, cnt);
}

int launch_f32_to_pcm16(const float* x, const int64_t* in_off, const int64_t* in_len, int n_files, int64_t max_len,
                        int16_t* q, const int64_t* out_off, int64_t out_stride, int* clipped, hipStream_t st) {
  if (n_files <= 0) return 0;
  if (out_stride < 1 || n_files > 65535) {
    set_error("f32_to_pcm16: need out_stride >= 1 and at most 65535 files");
    return -2;
  }
  NC_HIP(hipMemsetAsync(clipped, 0, (size_t)n_files * sizeof(int), st));
  if (max_len <= 0) return 0;
  const int gx = (int)std::max<int64_t>(1, std::min<int64_t>((max_len + 255) / 256, 256 * 16));
  hipLaunchKernelGGL(f32_to_pcm16_kernel, dim3(gx, n_files), dim3(256), 0, st, x, in_off, in_len, q, out_off,
                     out_stride, clipped);
  NC_HIP(hipGetLastError());
  return 0;
}

}  // namespace nc
