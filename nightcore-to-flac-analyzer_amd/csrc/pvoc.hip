// pvoc.hip — phase-vocoder time stretch, the device half of the pitch shift (what the
// reference's workflow shells out to `rubberband --pitch S` for, workflow.py:121-131; the other
// half is the speed render of speed.hip at the same ratio).  PARITY UNPINNED: rubberband is
// absent and the reference holds no pitch shifter; the definition is the project's own
// (DESIGN.md §4 "Pitch shift", tests/pvoc_ref.py).  Plain phase vocoder: no transient
// detection, no phase locking (identity phase locking with linked channels is opt-in: the last
// section of this file).
//   N = 2048, Hs = 512, Q = 1e6, W = periodic Hann, P = round(2^(S/12) Q) in [Q/2, 2Q],
//   Ns = ceil(n P / Q), K = ceil(Ns / Hs) + 3 frames, u_k = ((k - 1) Hs Q) div P (floor),
//   A_k = rfft(x[u_k - N/2 + i] W[i]), B_k the frame Hs samples earlier, mag_k = |A_k|,
//   empty_k = every x[i], u_k - N/2 < i < u_k + N/2, is +-0;  reset_k = k == 0 or empty_{k-1},
//   V_k = ph(A_k) on a reset frame, else ph(A_k conj B_k)        ph(z) = z / |z|, (1, 0) at 0 / inf
//   Phi_k = V_k on a reset frame, else ph(Phi_{k-1} V_k)
//   f_k[i] = irfft(mag_k Phi_k)[i] W[i] 2/3,  s[m] = sum_{k = j..j+3} f_k[m - (k - 3) Hs], j = m div Hs.
//
// MI355X layout, six launches whatever the lengths:
//   pv_analysis   persistent workgroups of 8 waves, one frame per wave from the workgroup's LDS
//                 queue (the stft_mel / spectral_frames scheme).  The 2560-sample span of B and A
//                 is loaded once (20 float2 per lane: B is rows 0..15, A rows 4..19 of the same
//                 registers), the empty test runs on those registers, each 2048-point real FFT is
//                 the 1024-point complex wave FFT of nc_device.h plus the mirror-paired real
//                 split; B's spectrum waits in a second LDS row.  mag and V leave as coalesced
//                 [frame][1025] rows (IEEE sqrt and divide).
//   pv_scan_tile / pv_scan_carry / pv_scan_apply   the segmented scan over frames, lanes along
//                 bins (row loads coalesce): tiles of PV_TILE frames multiply up in f64, one
//                 thread per (file, bin) walks the tile aggregates, the apply pass starts each
//                 tile from its carry.  The association is fixed by (file, frame index) alone.
//   pv_synth      one frame per wave: Y = mag Phi packed for the conjugate-trick inverse (a
//                 forward FFT of conj Z), window, 2/3, into a frame buffer [frame][2048].
//   pv_ola        every stretched sample adds its four frames in ascending k (f32 gather), and
//                 peak[file] = max |s| (atomic maximum on the bit pattern: order-free).
// The frame buffer + gather form was chosen for its fixed, atomic-free sum order; the variant
// that keeps a workgroup's last three frames in LDS was not built.
// No float atomics, no allocation, no host synchronisation; results are bit-identical run to run
// and batch to single.
#include <algorithm>

#include "nc_device.h"
#include "nc_launch.h"
#include "nc_ws.h"

namespace nc {

constexpr int PV_N = 2048;
constexpr int PV_HS = 512;
constexpr int PV_BINS = PV_N / 2 + 1;
constexpr int64_t PV_Q = 1000000;
constexpr int PV_TILE = 64;  // frames per scan tile
constexpr int PV_WAVES = 8;
constexpr int PV_THREADS = PV_WAVES * 64;
constexpr int PV_SPEC = 1032;  // float2 per spectrum row in LDS (1025, padded)
constexpr int64_t PV_MAX_N = INT64_C(1) << 40;
using PvTw = StagedTw<1024>;

__host__ __device__ inline int64_t pv_stretched_len(int64_t n, int64_t P) {
  return n <= 0 ? 0 : (n * P + PV_Q - 1) / PV_Q;
}
__host__ __device__ inline int64_t pv_frames(int64_t ns) { return ns <= 0 ? 0 : (ns + PV_HS - 1) / PV_HS + 3; }
// u_k = ((k - 1) Hs Q) div P, floor for k = 0 too
__device__ __forceinline__ int64_t pv_centre(int64_t k, int64_t P) {
  const int64_t c = (k - 1) * PV_HS * PV_Q;
  return c >= 0 ? c / P : -((-c + P - 1) / P);
}
__host__ __device__ inline int pv_al4(int n) { return (n + 3) & ~3; }
__host__ __device__ inline int64_t pv_scan_rows(int64_t total_frames, int n_files) {
  return total_frames / PV_TILE + n_files + 1;
}
// first aggregate row of a file whose frames start at fb: rows of different files never overlap
// (floor(a + b) >= floor(a) + floor(b), and the + f leaves room for every file's partial tile)
__device__ __forceinline__ int64_t pv_row0(int64_t fb, int f) { return fb / PV_TILE + f; }

struct PvScanWs {
  double2 *agg, *carry;  // [row][bin] tile aggregates, Phi of the frame before each tile
  uint8_t* aflag;        // [row]
};
static PvScanWs pv_scan_ws(WsCarve& c, int64_t total_frames, int n_files) {
  const size_t rows = (size_t)pv_scan_rows(total_frames, n_files);
  return {c.take<double2>(rows * PV_BINS), c.take<double2>(rows * PV_BINS), c.take<uint8_t>(rows)};  // member order
}
size_t pv_scan_ws_bytes(int64_t total_frames, int n_files) {
  WsCarve c;
  pv_scan_ws(c, total_frames, n_files);
  return c.bytes();
}

// The six sections of nc_pv_stretch's workspace, in bytes: mag, V, Phi, frame buffer, empty, scan
// workspace.  pv_plan lays them out 256-byte aligned; launch_pv_stretch holds the caller's
// offsets against them.
static void pv_stretch_sizes(int64_t total_frames, int n_files, size_t sizes[6]) {
  const size_t t = (size_t)total_frames;
  sizes[0] = t * PV_BINS * sizeof(float);
  sizes[1] = sizes[2] = t * PV_BINS * sizeof(float2);
  sizes[3] = t * PV_N * sizeof(float);
  sizes[4] = t;
  sizes[5] = pv_scan_ws_bytes(total_frames, n_files);
}

// Host plan: ns / k per file, frame_base [n_files + 1], and the workspace of nc_pv_stretch:
// ws_off[0..5] = mag, V, Phi, frame buffer, empty, scan workspace (bytes).
int pv_plan(int64_t P, const int64_t* n_in, int n_files, int64_t* ns_out, int64_t* k_out, int64_t* frame_base,
            int64_t* ws_off, size_t* ws_bytes) {
  if (P < PV_Q / 2 || P > 2 * PV_Q) {
    set_error("pv_plan: ratio outside [0.5, 2] (P = round(2^(S/12) 1e6), |S| <= 12)");
    return -2;
  }
  if (n_files < 0 || n_files > 65535 || (n_files > 0 && !n_in)) {
    set_error("pv_plan: need 0 .. 65535 files and their lengths");
    return -2;
  }
  int64_t total = 0;
  for (int f = 0; f < n_files; ++f) {
    if (n_in[f] < 0 || n_in[f] > PV_MAX_N) {
      set_error("pv_plan: input length outside 0 .. 2^40");
      return -2;
    }
    const int64_t ns = pv_stretched_len(n_in[f], P), k = pv_frames(ns);
    if (ns_out) ns_out[f] = ns;
    if (k_out) k_out[f] = k;
    if (frame_base) frame_base[f] = total;
    total += k;
  }
  if (frame_base) frame_base[n_files] = total;
  size_t sizes[6];
  pv_stretch_sizes(total, n_files, sizes);
  WsCarve c;
  for (int i = 0; i < 6; ++i) {
    if (ws_off) ws_off[i] = (int64_t)c.bytes();
    c.skip(sizes[i]);
  }
  if (ws_bytes) *ws_bytes = c.bytes();
  return 0;
}

// every file sample x[i], u - N/2 < i < u + N/2, is +-0 (wave-uniform)
__device__ __forceinline__ bool pv_span_empty(const float* x, int64_t L, int64_t u, int lane) {
  const int64_t lo = max(u - (PV_N / 2 - 1), (int64_t)0), hi = min(u + (PV_N / 2 - 1), L - 1);
  bool nz = false;
  for (int64_t i = lo + lane; i <= hi; i += 64) nz |= x[i] != 0.0f;
  return __ballot(nz) == 0;
}

// rfft of the 2048 windowed samples held as rows R0 .. R0 + 15 of xv (row r: samples
// 2 (lane + 64 r), + 1 of the span), into spec[0 .. 1024] (LDS; may be fftbuf itself)
template <int R0>
__device__ __forceinline__ void pv_rfft(const float2 (&xv)[20], const float2* __restrict__ hann2, float2* fftbuf,
                                        const float2* sh_tw, int lane, float2* spec) {
  FftIn<1024> in;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const float2 h = hann2[lane + 64 * r];
    in[0][r] = make_float2(xv[R0 + r].x * h.x, xv[R0 + r].y * h.y);
  }
  stockham_stage_regs<1024, 16, 1, 64, false, 0, 0>(in, fftbuf, sh_tw, lane);
  stockham_stage<1024, 16, 16, 64, false, 0, 0>(fftbuf, sh_tw, lane);
  float2 v[4][4];
  fft1024_last_mirror<PvTw::s3>(fftbuf, sh_tw, lane, v);  // all reads of fftbuf are complete
  rsplit_mirror<PvTw::split, true, true>(v, sh_tw, lane, [&](int k, float2 X, float2 XN) {
    spec[k] = X;
    spec[1024 - k] = XN;
  });
  asm volatile("" ::: "memory");  // the rows are read across lanes next (one wave: LDS runs in order)
}

__device__ __forceinline__ float2 pv_ph(float2 z, float m) {
  const bool ok = m > 0.0f && m < INFINITY;
  return ok ? make_float2(__fdiv_rn(z.x, m), __fdiv_rn(z.y, m)) : make_float2(1.0f, 0.0f);
}

struct PvAnaArgs {
  const float* x;
  const int64_t* in_off;
  const int64_t* in_len;
  const int64_t* frame_base;
  int n_files;
  int64_t total_frames;
  int64_t P;
  float* mag;
  float2* V;
  uint8_t* empty;
  const float2* tw;
  const float* hann;
  unsigned long long* span;
  float2* U;  // WITH_U only: ph(A_k); V may then be null (B_k is not transformed)
};

static size_t pv_analysis_lds() {
  return ((size_t)pv_al4(PvTw::size) + (size_t)PV_WAVES * (LdsSize<1024>::value + PV_SPEC)) * sizeof(float2);
}
static size_t pv_synth_lds() {
  return ((size_t)pv_al4(PvTw::size) + (size_t)PV_WAVES * LdsSize<1024>::value) * sizeof(float2);
}

// WITH_U: the analysis phasor U_k = ph(A_k) leaves as well (phase locking, below); mag, V and empty
// are computed by the same instructions in both variants.
template <bool WITH_U>
__global__ __launch_bounds__(PV_THREADS) void pv_analysis_kernel(PvAnaArgs a) {
  const Span span_(a.span);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float2* sh_tw = reinterpret_cast<float2*>(smem);
  const int lane0 = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float2* fftbuf = sh_tw + pv_al4(PvTw::size) + wave * (LdsSize<1024>::value + PV_SPEC);
  float2* spec_b = fftbuf + LdsSize<1024>::value;

  __shared__ int sh_next;  // the workgroup's frame queue (WgFrameQueue)
  if (threadIdx.x == 0) sh_next = 0;
  fill_staged_tw<1024>(sh_tw, a.tw, threadIdx.x, PV_THREADS);
  __syncthreads();

  const float2* hann2 = reinterpret_cast<const float2*>(a.hann);
  WgFrameQueue fq(&sh_next, lane0, a.total_frames, PV_WAVES);
  for (;;) {
    const int64_t g = fq.take(lane0);
    if (g >= fq.f1) break;
    const int f = uniform32(seg_of(a.frame_base, a.n_files, g));
    const int64_t k = g - uniform64(a.frame_base[f]);
    const int64_t L = uniform64(a.in_len[f]);
    const float* x = a.x + uniform64(a.in_off[f]);
    const int64_t u = pv_centre(k, a.P);

    int lane = lane0;
    asm volatile("" : "+v"(lane));
    // the span of B and A: samples u - N/2 - Hs + 2 (lane + 64 r) (+ 1), r < 20; zero outside the file
    const int64_t s0 = u - PV_N / 2 - PV_HS;
    float2 xv[20];
    bool nz = false;
#pragma unroll
    for (int r = 0; r < 20; ++r) {
      const int64_t i0 = s0 + 2 * (lane + 64 * r);
      const float x0 = (i0 >= 0 && i0 < L) ? x[i0] : 0.0f;
      const float x1 = (i0 + 1 >= 0 && i0 + 1 < L) ? x[i0 + 1] : 0.0f;
      xv[r] = make_float2(x0, x1);
      // A's samples 1 .. N - 1 (its sample 0, weight W[0] = 0, is not part of the test)
      if (r >= 4) nz |= (x0 != 0.0f && !(r == 4 && lane == 0)) || x1 != 0.0f;
    }
    const bool empty = __ballot(nz) == 0;
    const bool reset = k == 0 || pv_span_empty(x, L, pv_centre(k - 1, a.P), lane);
    if (lane == 0) a.empty[g] = empty ? 1 : 0;

    const bool with_v = !WITH_U || a.V != nullptr;  // kernel-uniform
    if (!reset && with_v) pv_rfft<0>(xv, hann2, fftbuf, sh_tw, lane, spec_b);
    pv_rfft<4>(xv, hann2, fftbuf, sh_tw, lane, fftbuf);
    const float2* spec_a = fftbuf;

    float* mrow = a.mag + g * PV_BINS;
    float2* vrow = a.V + g * PV_BINS;
    auto bin = [&](int b) {
      const float2 A = spec_a[b];
      const float ma = __fsqrt_rn(fmaf(A.x, A.x, A.y * A.y));
      mrow[b] = ma;
      if (WITH_U) a.U[g * PV_BINS + b] = pv_ph(A, ma);
      if (!with_v) return;
      float2 v;
      if (reset) {
        v = pv_ph(A, ma);
      } else {
        const float2 B = spec_b[b];
        const float2 z = make_float2(fmaf(A.x, B.x, A.y * B.y), fmaf(A.y, B.x, -(A.x * B.y)));
        v = pv_ph(z, __fsqrt_rn(fmaf(z.x, z.x, z.y * z.y)));
      }
      vrow[b] = v;
    };
#pragma unroll
    for (int j = 0; j < 16; ++j) bin(lane + 64 * j);
    if (lane == 0) bin(1024);
    asm volatile("" ::: "memory");  // the next frame's exchanges overwrite the rows read here
  }
}

int launch_pv_analyze(Context& ctx, const float* x, const int64_t* in_off, const int64_t* in_len,
                      const int64_t* frame_base, int n_files, int64_t total_frames, int64_t P, float* mag, float2* V,
                      uint8_t* empty, float2* U, bool with_u, hipStream_t st) {
  if (P < PV_Q / 2 || P > 2 * PV_Q) {
    set_error("pv_analyze: ratio outside [0.5, 2]");
    return -2;
  }
  if (n_files < 0 || n_files > 65535 || total_frames < 0) {
    set_error("pv_analyze: need 0 .. 65535 files and total_frames >= 0");
    return -2;
  }
  if (n_files == 0 || total_frames == 0) return 0;
  if (!x || !in_off || !in_len || !frame_base || !mag || (!V && !with_u) || !empty || (with_u && !U)) {
    set_error("pv_analyze: null argument");
    return -2;
  }
  PvAnaArgs a{x, in_off, in_len, frame_base, n_files, total_frames, P, mag, V, empty, ctx.t.tw, ctx.t.hann2048, nullptr,
              with_u ? U : nullptr};
  const int64_t n_groups = (total_frames + PV_WAVES - 1) / PV_WAVES;
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(n_groups, ctx.num_cu));
  {
    KTimer kt_(ctx, "pv_analysis", st);
    a.span = kt_.span();
    if (with_u)
      hipLaunchKernelGGL(pv_analysis_kernel<true>, dim3(grid), dim3(PV_THREADS), pv_analysis_lds(), st, a);
    else
      hipLaunchKernelGGL(pv_analysis_kernel<false>, dim3(grid), dim3(PV_THREADS), pv_analysis_lds(), st, a);
  }
  NC_HIP(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------------ phase scan
// (r1, v1) o (r2, v2) = (r1 | r2, r2 ? v2 : v1 v2) over the frames of one bin, in f64.
struct PvScanArgs {
  const float2* V;
  const uint8_t* empty;
  const int64_t* frame_base;
  float2* phi;
  double2* agg;    // [row][bin] tile aggregates
  double2* carry;  // [row][bin] the value entering each tile
  uint8_t* aflag;  // [row] the tile holds a reset
  unsigned long long* span;
};

__device__ __forceinline__ double2 pv_mul(double2 p, float2 v) {
  return make_double2(p.x * (double)v.x - p.y * (double)v.y, p.x * (double)v.y + p.y * (double)v.x);
}
__device__ __forceinline__ double2 pv_ph64(double2 p) {
  const double m = sqrt(p.x * p.x + p.y * p.y);
  return (m > 0.0 && m < (double)INFINITY) ? make_double2(p.x / m, p.y / m) : make_double2(1.0, 0.0);
}

// grid (bin blocks, tiles, files); MODE 0: tile aggregates, MODE 1: apply from the carries
template <int MODE>
__global__ __launch_bounds__(256) void pv_scan_tile_kernel(PvScanArgs a) {
  const Span span_(a.span);
  const int b = blockIdx.x * 256 + threadIdx.x, t = blockIdx.y, f = blockIdx.z;
  const int64_t fb = a.frame_base[f], K = a.frame_base[f + 1] - fb;
  const int64_t k0 = (int64_t)t * PV_TILE;
  if (k0 >= K || b >= PV_BINS) return;
  const int64_t k1 = min(K, k0 + PV_TILE);
  const int64_t row = pv_row0(fb, f) + t;
  double2 p = MODE ? a.carry[row * PV_BINS + b] : make_double2(1.0, 0.0);
  bool fl = false;
  for (int64_t k = k0; k < k1; ++k) {
    const bool reset = k == 0 || a.empty[fb + k - 1] != 0;
    const float2 v = a.V[(fb + k) * PV_BINS + b];
    if (reset) {
      p = make_double2((double)v.x, (double)v.y);
      fl = true;
      if (MODE) a.phi[(fb + k) * PV_BINS + b] = v;
    } else {
      p = pv_mul(p, v);
      if (MODE) {
        const double2 q = pv_ph64(p);
        a.phi[(fb + k) * PV_BINS + b] = make_float2((float)q.x, (float)q.y);
      }
    }
  }
  if (!MODE) {
    a.agg[row * PV_BINS + b] = p;
    if (b == 0) a.aflag[row] = fl ? 1 : 0;
  }
}

// grid (bin blocks, files): the exclusive scan of a file's tile aggregates, tile after tile
__global__ __launch_bounds__(256) void pv_scan_carry_kernel(PvScanArgs a) {
  const Span span_(a.span);
  const int b = blockIdx.x * 256 + threadIdx.x, f = blockIdx.y;
  if (b >= PV_BINS) return;
  const int64_t fb = a.frame_base[f], K = a.frame_base[f + 1] - fb;
  const int64_t tiles = (K + PV_TILE - 1) / PV_TILE, row0 = pv_row0(fb, f);
  double2 c = make_double2(1.0, 0.0);
  for (int64_t t = 0; t < tiles; ++t) {
    const int64_t i = (row0 + t) * PV_BINS + b;
    a.carry[i] = c;
    const double2 g = a.agg[i];
    const double2 m = make_double2(c.x * g.x - c.y * g.y, c.x * g.y + c.y * g.x);
    c = pv_ph64(a.aflag[row0 + t] ? g : m);
  }
}

int launch_pv_scan(Context& ctx, const float2* V, const uint8_t* empty, const int64_t* frame_base, int n_files,
                   int64_t total_frames, int64_t max_frames, float2* phi, void* ws, size_t ws_bytes, hipStream_t st) {
  if (n_files < 0 || n_files > 65535 || total_frames < 0 || max_frames < 0 || max_frames > total_frames) {
    set_error("pv_scan: need 0 .. 65535 files and 0 <= max_frames <= total_frames");
    return -2;
  }
  if (n_files == 0 || total_frames == 0) return 0;
  if (!V || !empty || !frame_base || !phi || !ws) {
    set_error("pv_scan: null argument");
    return -2;
  }
  WsCarve c(ws);
  const PvScanWs w = pv_scan_ws(c, total_frames, n_files);
  if (ws_bytes < c.bytes()) {
    set_error("pv_scan: workspace below nc_pv_plan's scan size");
    return -2;
  }
  const int64_t max_tiles = (max_frames + PV_TILE - 1) / PV_TILE;
  if (max_tiles < 1 || max_tiles > 65535 || ((uintptr_t)ws & 15)) {
    set_error("pv_scan: max_frames must be the longest file's frame count (1 .. 65535 tiles), ws 16-byte aligned");
    return -2;
  }
  PvScanArgs a{V, empty, frame_base, phi, w.agg, w.carry, w.aflag, nullptr};
  const unsigned bx = (PV_BINS + 255) / 256;
  const dim3 gt(bx, (unsigned)max_tiles, (unsigned)n_files);
  {
    KTimer kt_(ctx, "pv_scan_tile", st);
    a.span = kt_.span();
    hipLaunchKernelGGL(pv_scan_tile_kernel<0>, gt, dim3(256), 0, st, a);
  }
  {
    KTimer kt_(ctx, "pv_scan_carry", st);
    a.span = kt_.span();
    hipLaunchKernelGGL(pv_scan_carry_kernel, dim3(bx, (unsigned)n_files), dim3(256), 0, st, a);
  }
  {
    KTimer kt_(ctx, "pv_scan_apply", st);
    a.span = kt_.span();
    hipLaunchKernelGGL(pv_scan_tile_kernel<1>, gt, dim3(256), 0, st, a);
  }
  NC_HIP(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------------ synthesis
struct PvSynArgs {
  const float* mag;
  const float2* phi;
  int64_t total_frames;
  float* frames;  // [frame][2048]
  const float2* tw;
  const float* hann;
  unsigned long long* span;
};

// irfft by the conjugate trick: with X = mag Phi (bins 0 and 1024 real), w = exp(-2 pi i / 2048),
//   E[k] = X[k] + conj X[1024 - k],  O[k] = (X[k] - conj X[1024 - k]) conj(w^k),  Z = E + i O,
//   x[2 n] + i x[2 n + 1] = conj(FFT_1024(conj Z))[n] / 2048.
__global__ __launch_bounds__(PV_THREADS) void pv_synth_kernel(PvSynArgs a) {
  const Span span_(a.span);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float2* sh_tw = reinterpret_cast<float2*>(smem);
  const int lane0 = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float2* fftbuf = sh_tw + pv_al4(PvTw::size) + wave * LdsSize<1024>::value;
  __shared__ int sh_next;  // the workgroup's frame queue (WgFrameQueue)
  if (threadIdx.x == 0) sh_next = 0;
  fill_staged_tw<1024>(sh_tw, a.tw, threadIdx.x, PV_THREADS);
  __syncthreads();

  const float2* hann2 = reinterpret_cast<const float2*>(a.hann);
  WgFrameQueue fq(&sh_next, lane0, a.total_frames, PV_WAVES);
  for (;;) {
    const int64_t g = fq.take(lane0);
    if (g >= fq.f1) break;
    int lane = lane0;
    asm volatile("" : "+v"(lane));
    const float* mrow = a.mag + g * PV_BINS;
    const float2* prow = a.phi + g * PV_BINS;
    FftIn<1024> in;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int k = lane + 64 * r;
      const float m0 = mrow[k], m1 = mrow[1024 - k];
      const float2 p0 = prow[k], p1 = prow[1024 - k];
      float2 X = make_float2(m0 * p0.x, m0 * p0.y), XN = make_float2(m1 * p1.x, m1 * p1.y);
      if (k == 0) X.y = XN.y = 0.0f;  // numpy's irfft ignores the imaginary parts of bins 0 and N/2
      const float2 E = make_float2(X.x + XN.x, X.y - XN.y);
      const float2 O = cmul(make_float2(X.x - XN.x, X.y + XN.y), cconj(a.tw[4 * k]));
      in[0][r] = make_float2(E.x - O.y, -(E.y + O.x));  // conj(E + i O)
    }
    wave_fft<1024, 0>(in, fftbuf, sh_tw, lane);
    asm volatile("" ::: "memory");  // natural-order output read across lanes (one wave: in order)
    float2* out = reinterpret_cast<float2*>(a.frames + g * PV_N);
    const float inv = 1.0f / 2048.0f, c23 = (float)(2.0 / 3.0);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int n = lane + 64 * j;
      const float2 F = fftbuf[lpad(n)];
      const float2 h = hann2[n];
      out[n] = make_float2(__fmul_rn(__fmul_rn(__fmul_rn(F.x, inv), h.x), c23),
                           __fmul_rn(__fmul_rn(__fmul_rn(-F.y, inv), h.y), c23));
    }
    asm volatile("" ::: "memory");
  }
}

// s[m] = sum of the four frames over stretched sample m, ascending k; grid (blocks, files), a
// workgroup of 256 threads covers PV_OLA_OUT samples.  One sample per thread ran 749 us on a 3-min
// stereo file, bound by its 32 858 peak atomics per file on one address; 16 per thread: see DESIGN.md.
constexpr int PV_OLA_OUT = 4096;
__global__ __launch_bounds__(256) void pv_ola_kernel(const float* __restrict__ frames,
                                                     const int64_t* __restrict__ in_len,
                                                     const int64_t* __restrict__ frame_base, int64_t P,
                                                     float* __restrict__ s_all, const int64_t* __restrict__ out_off,
                                                     unsigned* peak, unsigned long long* span) {
  const Span span_(span);
  __shared__ float red[4];
  const int f = blockIdx.y;
  const int64_t ns = pv_stretched_len(in_len[f], P);
  const int64_t fb = frame_base[f], K = frame_base[f + 1] - fb;
  const int64_t m0 = (int64_t)blockIdx.x * PV_OLA_OUT;
  if (m0 >= ns) return;
  float* s = s_all + out_off[f];
  float pk = 0.0f;
#pragma unroll 4
  for (int o = 0; o < PV_OLA_OUT / 256; ++o) {
    const int64_t m = m0 + o * 256 + threadIdx.x;
    if (m < ns) {
      const int64_t j = m / PV_HS;
      const int i = (int)(m - j * PV_HS);
      float acc = 0.0f;
      if (j + 3 < K) {  // always, when frame_base is nc_pv_plan's
        const float* fr = frames + (fb + j) * PV_N + i;
        acc = fr[3 * PV_HS];
        acc += fr[PV_N + 2 * PV_HS];
        acc += fr[2 * PV_N + PV_HS];
        acc += fr[3 * PV_N];
      }
      s[m] = acc;
      pk = fmaxf(pk, fabsf(acc));
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) pk = fmaxf(pk, __shfl_xor(pk, d, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = pk;
  __syncthreads();
  if (threadIdx.x == 0)
    atomicMax(peak + f, __float_as_uint(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]))));
}

int launch_pv_synth(Context& ctx, const float* mag, const float2* phi, const int64_t* in_len,
                    const int64_t* frame_base, int n_files, int64_t total_frames, int64_t P, int64_t max_ns,
                    float* frames, size_t frames_bytes, float* s, const int64_t* out_off, float* peak,
                    hipStream_t st) {
  if (P < PV_Q / 2 || P > 2 * PV_Q) {
    set_error("pv_synth: ratio outside [0.5, 2]");
    return -2;
  }
  if (n_files < 0 || n_files > 65535 || total_frames < 0 || max_ns < 0 ||
      max_ns > (int64_t)PV_HS * std::max<int64_t>(0, total_frames - 3)) {
    set_error("pv_synth: need 0 .. 65535 files and 0 <= max_ns <= 512 (total_frames - 3)");
    return -2;
  }
  if (n_files == 0) return 0;
  if (!peak) {
    set_error("pv_synth: null peak");
    return -2;
  }
  NC_HIP(hipMemsetAsync(peak, 0, (size_t)n_files * sizeof(float), st));
  if (total_frames == 0 || max_ns == 0) return 0;
  if (!mag || !phi || !in_len || !frame_base || !frames || !s || !out_off) {
    set_error("pv_synth: null argument");
    return -2;
  }
  if (frames_bytes < (size_t)total_frames * PV_N * sizeof(float)) {
    set_error("pv_synth: frame buffer below 8192 bytes per frame");
    return -2;
  }
  if ((max_ns + PV_OLA_OUT - 1) / PV_OLA_OUT > 0x7fffffff) {
    set_error("pv_synth: too many outputs for one launch");
    return -2;
  }
  PvSynArgs a{mag, phi, total_frames, frames, ctx.t.tw, ctx.t.hann2048, nullptr};
  const int64_t n_groups = (total_frames + PV_WAVES - 1) / PV_WAVES;
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(n_groups, 2 * (int64_t)ctx.num_cu));
  {
    KTimer kt_(ctx, "pv_synth", st);
    a.span = kt_.span();
    hipLaunchKernelGGL(pv_synth_kernel, dim3(grid), dim3(PV_THREADS), pv_synth_lds(), st, a);
  }
  {
    KTimer kt_(ctx, "pv_ola", st);
    hipLaunchKernelGGL(pv_ola_kernel, dim3((unsigned)((max_ns + PV_OLA_OUT - 1) / PV_OLA_OUT), (unsigned)n_files),
                       dim3(256), 0, st,
                       frames, in_len, frame_base, P, s, out_off, reinterpret_cast<unsigned*>(peak), kt_.span());
  }
  NC_HIP(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------------ phase locking
// Identity phase locking with linked channels (opt-in; DESIGN.md §4 "Phase locking",
// tests/pvoc_lock_ref.py).  With U_k = ph(A_k):
//   peaks    b is a peak iff mag[b] > mag[b-1], mag[b-2] and mag[b] >= mag[b+1], mag[b+2] (neighbours
//            outside 0..1024 ignored); a frame without one has the single peak 0
//   owners   o_k[b]: between consecutive peaks p < q, b <= (p + q) div 2 belongs to p, the rest to q
//   M_k[b] = V_k[b] when b == o (and on a reset frame), else V_k[o] U_k[b] conj(U_k[o])
//   Phi_k  = V_k on a reset frame, else Phi_k[b] = ph(Phi_{k-1}[o_k[b]] M_k[b])
//   linked   the channels of a group follow the scan Psi of their float32 sum m:
//            Phi^c_k[b] = ph(Psi_k[b] U^c_k[b] conj(U^m_k[b])); a group of one channel is Psi itself.
//   pv_lock_prep   one wave per frame, lanes along bins: the peak test leaves as 17 ballots (the
//                  frame's peak bitmap in SGPRs), the nearest peak below and above each bin comes
//                  from clz / ffs on its word; writes owner (uint16) and M (f64 product, stored f32).
//   pv_lock_tile / pv_lock_carry / pv_lock_apply   the plain scan's three passes, generalised by a
//                  source bin: a workgroup walks the PV_TILE frames of one (file, tile) with the
//                  whole row in LDS (double-buffered: frame k gathers from frame k - 1's row); each
//                  bin carries (source bin at the tile start or PV_ABS after a reset, f64 product).
//                  One workgroup per file walks the tile aggregates with the same gather.
//   pv_mid_sum / pv_rotate   the linked channels' sum, and their phases from Psi (bandwidth).
// Fixed launch counts, no atomics, no allocation, no host synchronisation; the association depends
// on the file's own frame index alone.
constexpr unsigned PV_ABS = 0xffffu;  // source marker: the product is absolute (a reset was met)
constexpr int PV_LROW = PV_BINS + 3;  // LDS row stride
constexpr int PV_LBPT = 5;            // bins per thread of a 256-thread workgroup (5 x 256 >= 1025)
constexpr int PV_CDEPTH = 4;          // tile aggregates in flight ahead of the carry walk

struct PvLockArgs {
  const float* mag;
  const float2* U;
  const float2* V;
  const uint8_t* empty;
  const int64_t* frame_base;
  int n_files;
  int64_t total_frames;
  uint16_t* owner;  // [frame][bin]
  float2* M;        // [frame][bin]
  float2* phi;
  double2* agg;     // [row][bin] tile aggregates
  uint16_t* asrc;   // [row][bin] their source bins
  double2* carry;   // [row][bin] Phi of the frame before each tile
  unsigned long long* span;
};

struct PvLockWs {
  float2* M;             // [frame][bin]
  uint16_t* owner;       // [frame][bin] (the slot stays reserved under a caller's owner array)
  double2 *agg, *carry;  // [row][bin]
  uint16_t* asrc;        // [row][bin]
};
static PvLockWs pv_lock_ws(WsCarve& c, int64_t total_frames, int n_files) {
  const size_t t = (size_t)total_frames, rows = (size_t)pv_scan_rows(total_frames, n_files);
  return {c.take<float2>(t * PV_BINS), c.take<uint16_t>(t * PV_BINS), c.take<double2>(rows * PV_BINS),
          c.take<double2>(rows * PV_BINS), c.take<uint16_t>(rows * PV_BINS)};  // member order, left to right
}
size_t pv_lock_ws_bytes(int64_t total_frames, int n_files) {
  WsCarve c;
  pv_lock_ws(c, total_frames, n_files);
  return c.bytes();
}

__device__ __forceinline__ double2 pv_mul64(double2 p, double2 v) {
  return make_double2(p.x * v.x - p.y * v.y, p.x * v.y + p.y * v.x);
}

__global__ __launch_bounds__(256) void pv_lock_prep_kernel(PvLockArgs a) {
  const Span span_(a.span);
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t g = (int64_t)blockIdx.x * 4 + wave;
  if (g >= a.total_frames) return;
  const int f = uniform32(seg_of(a.frame_base, a.n_files, g));
  const bool reset = g == uniform64(a.frame_base[f]) || a.empty[g - 1] != 0;
  const float* m = a.mag + g * PV_BINS;

  unsigned long long mask[17];
  bool any = false;
#pragma unroll
  for (int j = 0; j < 17; ++j) {
    const int b = 64 * j + lane;
    bool pk = false;
    if (b < PV_BINS) {
      const float m0 = m[b];
      pk = (b < 1 || m0 > m[b - 1]) && (b < 2 || m0 > m[b - 2]) && (b + 1 >= PV_BINS || m0 >= m[b + 1]) &&
           (b + 2 >= PV_BINS || m0 >= m[b + 2]);
    }
    mask[j] = __ballot(pk);
    any |= mask[j] != 0;
  }
  if (!any) mask[0] = 1;  // non-finite magnitudes only: the single peak 0
  // the nearest peak in the words below / above each word (-1: none)
  int below[17], above[17];
  int last = -1;
#pragma unroll
  for (int j = 0; j < 17; ++j) {
    below[j] = last;
    if (mask[j]) last = 64 * j + 63 - __clzll((long long)mask[j]);
  }
  last = -1;
#pragma unroll
  for (int j = 16; j >= 0; --j) {
    above[j] = last;
    if (mask[j]) last = 64 * j + __ffsll((long long)mask[j]) - 1;
  }

  const float2* V = a.V + g * PV_BINS;
  const float2* U = a.U + g * PV_BINS;
#pragma unroll
  for (int j = 0; j < 17; ++j) {
    const int b = 64 * j + lane;
    if (b >= PV_BINS) continue;
    const unsigned long long lo = mask[j] & (~0ull >> (63 - lane)), hi = mask[j] & (~0ull << lane);
    const int p = lo ? 64 * j + 63 - __clzll((long long)lo) : below[j];
    const int q = hi ? 64 * j + __ffsll((long long)hi) - 1 : above[j];
    const int o = p < 0 ? q : (q < 0 ? p : (b <= ((p + q) >> 1) ? p : q));  // a peak: p == q == b
    a.owner[g * PV_BINS + b] = (uint16_t)o;
    float2 M = V[b];
    if (!reset && o != b) {
      const float2 vo = V[o], uo = U[o], ub = U[b];
      const double2 r = pv_mul64(make_double2((double)ub.x, (double)ub.y), make_double2((double)uo.x, -(double)uo.y));
      const double2 z = pv_mul64(make_double2((double)vo.x, (double)vo.y), r);
      M = make_float2((float)z.x, (float)z.y);
    }
    a.M[g * PV_BINS + b] = M;
  }
}

// grid (tiles, files); MODE 0: tile aggregates, MODE 1: apply from the carries
template <int MODE>
__global__ __launch_bounds__(256) void pv_lock_tile_kernel(PvLockArgs a) {
  const Span span_(a.span);
  __shared__ double2 sp[2][PV_LROW];
  __shared__ uint16_t ss[2][PV_LROW];
  const int t = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
  const int64_t fb = a.frame_base[f], K = a.frame_base[f + 1] - fb;
  const int64_t k0 = (int64_t)t * PV_TILE;
  if (k0 >= K) return;  // the whole workgroup
  const int64_t k1 = min(K, k0 + PV_TILE);
  const int64_t row = pv_row0(fb, f) + t;
#pragma unroll
  for (int i = 0; i < PV_LBPT; ++i) {
    const int b = tid + 256 * i;
    if (b < PV_BINS) {
      sp[0][b] = MODE ? a.carry[row * PV_BINS + b] : make_double2(1.0, 0.0);
      ss[0][b] = (uint16_t)b;
    }
  }
  float2 Mn[PV_LBPT];
  unsigned on[PV_LBPT];
  // loads without a branch around them (lanes past the row and the step past the tile read a
  // clamped address again): a guarded load makes the compiler drain every load at the join
  auto fetch = [&](int64_t k) {
    k = min(k, k1 - 1);
#pragma unroll
    for (int i = 0; i < PV_LBPT; ++i) {
      const int b = min(tid + 256 * i, PV_BINS - 1);
      Mn[i] = a.M[(fb + k) * PV_BINS + b];
      on[i] = a.owner[(fb + k) * PV_BINS + b];
    }
  };
  fetch(k0);
  __syncthreads();
  int cur = 0;
  for (int64_t k = k0; k < k1; ++k) {
    const bool reset = k == 0 || a.empty[fb + k - 1] != 0;
    float2 Mc[PV_LBPT];
    unsigned oc[PV_LBPT];
#pragma unroll
    for (int i = 0; i < PV_LBPT; ++i) {
      Mc[i] = Mn[i];
      oc[i] = on[i];
    }
    fetch(k + 1);
#pragma unroll
    for (int i = 0; i < PV_LBPT; ++i) {
      const int b = tid + 256 * i;
      if (b >= PV_BINS) continue;
      const int o = min(oc[i], (unsigned)(PV_BINS - 1));
      double2 p;
      unsigned s;
      if (reset) {
        p = make_double2((double)Mc[i].x, (double)Mc[i].y);
        s = PV_ABS;
      } else {
        p = pv_mul(sp[cur][o], Mc[i]);
        s = ss[cur][o];
      }
      sp[cur ^ 1][b] = p;
      ss[cur ^ 1][b] = (uint16_t)s;
      if (MODE) {
        float2 out = Mc[i];  // a reset frame: V itself
        if (!reset) {
          const double2 q = pv_ph64(p);
          out = make_float2((float)q.x, (float)q.y);
        }
        a.phi[(fb + k) * PV_BINS + b] = out;
      }
    }
    __syncthreads();
    cur ^= 1;
  }
  if (!MODE) {
#pragma unroll
    for (int i = 0; i < PV_LBPT; ++i) {
      const int b = tid + 256 * i;
      if (b < PV_BINS) {
        a.agg[row * PV_BINS + b] = sp[cur][b];
        a.asrc[row * PV_BINS + b] = ss[cur][b];
      }
    }
  }
}

// grid (files): Phi of the frame before each tile, tile after tile, by the aggregates' gather
__global__ __launch_bounds__(256) void pv_lock_carry_kernel(PvLockArgs a) {
  const Span span_(a.span);
  __shared__ double2 sc[2][PV_LROW];
  const int f = blockIdx.x, tid = threadIdx.x;
  const int64_t fb = a.frame_base[f], K = a.frame_base[f + 1] - fb;
  const int64_t tiles = (K + PV_TILE - 1) / PV_TILE, row0 = pv_row0(fb, f);
  if (tiles <= 0) return;
#pragma unroll
  for (int i = 0; i < PV_LBPT; ++i) {
    const int b = tid + 256 * i;
    if (b < PV_BINS) sc[0][b] = make_double2(1.0, 0.0);
  }
  // the aggregates do not depend on the chain: PV_CDEPTH tiles are in flight ahead of the walk
  double2 gq[PV_CDEPTH][PV_LBPT];
  unsigned sq[PV_CDEPTH][PV_LBPT];
  // (loads without a branch around them, as in the tile pass: clamped, re-reading the last tile)
  auto fetch = [&](int d, int64_t t) {
    t = min(t, tiles - 1);
#pragma unroll
    for (int i = 0; i < PV_LBPT; ++i) {
      const int b = min(tid + 256 * i, PV_BINS - 1);
      gq[d][i] = a.agg[(row0 + t) * PV_BINS + b];
      sq[d][i] = a.asrc[(row0 + t) * PV_BINS + b];
    }
  };
#pragma unroll
  for (int d = 0; d < PV_CDEPTH; ++d) fetch(d, d);
  __syncthreads();
  int cur = 0;
  for (int64_t t0 = 0; t0 < tiles; t0 += PV_CDEPTH) {
#pragma unroll
    for (int d = 0; d < PV_CDEPTH; ++d) {
      const int64_t t = t0 + d;
      if (t >= tiles) break;  // the whole workgroup
      double2 gc[PV_LBPT];
      unsigned scur[PV_LBPT];
#pragma unroll
      for (int i = 0; i < PV_LBPT; ++i) {
        gc[i] = gq[d][i];
        scur[i] = sq[d][i];
      }
      fetch(d, t + PV_CDEPTH);
#pragma unroll
      for (int i = 0; i < PV_LBPT; ++i) {
        const int b = tid + 256 * i;
        if (b >= PV_BINS) continue;
        a.carry[(row0 + t) * PV_BINS + b] = sc[cur][b];
        const bool abs_ = scur[i] >= (unsigned)PV_BINS;
        const double2 c = sc[cur][abs_ ? 0 : scur[i]];
        double2 n = abs_ ? gc[i] : pv_mul64(c, gc[i]);
        // a product of unit phasors: renormalised (an f64 square root and two divides, on the one CU
        // this file has) only once its length has left 1 +- 5e-4 or is not a number; the apply pass
        // normalises every Phi it stores, and a positive scale does not move a phase
        const double m2 = n.x * n.x + n.y * n.y;
        if (!(fabs(m2 - 1.0) < 1e-3)) n = pv_ph64(n);
        sc[cur ^ 1][b] = n;
      }
      __syncthreads();
      cur ^= 1;
    }
  }
}

int launch_pv_lock(Context& ctx, const float* mag, const float2* U, const float2* V, const uint8_t* empty,
                   const int64_t* frame_base, int n_files, int64_t total_frames, int64_t max_frames, float2* phi,
                   uint16_t* owner, void* ws, size_t ws_bytes, hipStream_t st) {
  if (n_files < 0 || n_files > 65535 || total_frames < 0 || max_frames < 0 || max_frames > total_frames) {
    set_error("pv_lock: need 0 .. 65535 files and 0 <= max_frames <= total_frames");
    return -2;
  }
  if (n_files == 0 || total_frames == 0) return 0;
  if (!mag || !U || !V || !empty || !frame_base || !phi || !ws) {
    set_error("pv_lock: null argument");
    return -2;
  }
  WsCarve c(ws);
  const PvLockWs w = pv_lock_ws(c, total_frames, n_files);
  if (ws_bytes < c.bytes()) {
    set_error("pv_lock: workspace below nc_pv_lock_ws_bytes");
    return -2;
  }
  const int64_t max_tiles = (max_frames + PV_TILE - 1) / PV_TILE;
  if (max_tiles < 1 || max_tiles > 0x7fffffff || ((uintptr_t)ws & 15) || (total_frames + 3) / 4 > 0x7fffffff) {
    set_error("pv_lock: max_frames must be the longest file's frame count (at least 1), ws 16-byte aligned");
    return -2;
  }
  PvLockArgs a{mag, U, V, empty, frame_base, n_files, total_frames, owner ? owner : w.owner, w.M, phi,
               w.agg, w.asrc, w.carry, nullptr};
  const dim3 gt((unsigned)max_tiles, (unsigned)n_files);
  {
    KTimer kt_(ctx, "pv_lock_prep", st);
    a.span = kt_.span();
    hipLaunchKernelGGL(pv_lock_prep_kernel, dim3((unsigned)((total_frames + 3) / 4)), dim3(256), 0, st, a);
  }
  {
    KTimer kt_(ctx, "pv_lock_tile", st);
    a.span = kt_.span();
    hipLaunchKernelGGL(pv_lock_tile_kernel<0>, gt, dim3(256), 0, st, a);
  }
  {
    KTimer kt_(ctx, "pv_lock_carry", st);
    a.span = kt_.span();
    hipLaunchKernelGGL(pv_lock_carry_kernel, dim3((unsigned)n_files), dim3(256), 0, st, a);
  }
  {
    KTimer kt_(ctx, "pv_lock_apply", st);
    a.span = kt_.span();
    hipLaunchKernelGGL(pv_lock_tile_kernel<1>, gt, dim3(256), 0, st, a);
  }
  NC_HIP(hipGetLastError());
  return 0;
}

// m[i] = ((x_0[i] + x_1[i]) + ...) in float32, channel order; grid (blocks, groups)
__global__ __launch_bounds__(256) void pv_mid_sum_kernel(const float* __restrict__ x,
                                                         const int64_t* __restrict__ sig_off,
                                                         const int64_t* __restrict__ sig_len,
                                                         const int* __restrict__ group_first, float* __restrict__ mid,
                                                         const int64_t* __restrict__ mid_off,
                                                         unsigned long long* span) {
  const Span span_(span);
  const int gr = blockIdx.y, c0 = group_first[gr], c1 = group_first[gr + 1];
  if (c1 <= c0) return;
  int64_t n = sig_len[c0];
  for (int c = c0 + 1; c < c1; ++c) n = min(n, sig_len[c]);  // equal by contract (checked on the host)
  float* out = mid + mid_off[gr];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    float acc = x[sig_off[c0] + i];
    for (int c = c0 + 1; c < c1; ++c) acc = __fadd_rn(acc, x[sig_off[c] + i]);
    out[i] = acc;
  }
}

int launch_pv_mid_sum(Context& ctx, const float* x, const int64_t* sig_off, const int64_t* sig_len,
                      const int* group_first, const int64_t* host_len, const int* host_first, int n_groups,
                      float* mid, const int64_t* mid_off, hipStream_t st) {
  if (n_groups < 0 || n_groups > 65535) {
    set_error("pv_mid_sum: need 0 .. 65535 groups");
    return -2;
  }
  if (n_groups == 0) return 0;
  if (!host_len || !host_first) {
    set_error("pv_mid_sum: null host lengths");
    return -2;
  }
  int64_t max_len = 0;
  for (int g = 0; g < n_groups; ++g) {
    if (host_first[g] < 0 || host_first[g + 1] <= host_first[g]) {
      set_error("pv_mid_sum: group_first must rise by at least one channel per group");
      return -2;
    }
    const int64_t n = host_len[host_first[g]];
    for (int c = host_first[g]; c < host_first[g + 1]; ++c)
      if (host_len[c] != n || n < 0) {
        set_error("pv_mid_sum: the channels of a group must be equally long");
        return -2;
      }
    max_len = std::max(max_len, n);
  }
  if (max_len == 0) return 0;
  if (!x || !sig_off || !sig_len || !group_first || !mid || !mid_off) {
    set_error("pv_mid_sum: null argument");
    return -2;
  }
  const unsigned bx = (unsigned)std::min<int64_t>((max_len + 1023) / 1024, 4096);
  {
    KTimer kt_(ctx, "pv_mid_sum", st);
    hipLaunchKernelGGL(pv_mid_sum_kernel, dim3(bx, (unsigned)n_groups), dim3(256), 0, st, x, sig_off, sig_len,
                       group_first, mid, mid_off, kt_.span());
  }
  NC_HIP(hipGetLastError());
  return 0;
}

struct PvRotArgs {
  const float2* psi;    // the groups' locked scans, rows laid out by mid_base
  const float2* u_mid;
  const int64_t* mid_base;  // [groups + 1]
  const float2* u;          // the channels' analysis phasors, rows laid out by frame_base
  const int64_t* frame_base;  // [files + 1]
  const int* group_first;     // [groups + 1]
  int n_files, n_groups;
  int64_t total_frames;
  float2* phi;
  unsigned long long* span;
};

// one wave per channel frame: Phi^c = ph(Psi U^c conj(U^m)) in f64; a group of one channel copies Psi
__global__ __launch_bounds__(256) void pv_rotate_kernel(PvRotArgs a) {
  const Span span_(a.span);
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t g = (int64_t)blockIdx.x * 4 + wave;
  if (g >= a.total_frames) return;
  const int c = uniform32(seg_of(a.frame_base, a.n_files, g));
  const int64_t k = g - uniform64(a.frame_base[c]);
  const int gr = uniform32(seg_of(a.n_groups, (int64_t)c, [&](int m) { return (int64_t)a.group_first[m]; }));
  const int64_t mb = uniform64(a.mid_base[gr]);
  if (k >= uniform64(a.mid_base[gr + 1]) - mb) return;  // never, when both plans are nc_pv_plan's
  const bool single = a.group_first[gr + 1] - a.group_first[gr] == 1;
  const float2* psi = a.psi + (mb + k) * PV_BINS;
  const float2* um = a.u_mid + (mb + k) * PV_BINS;
  const float2* u = a.u + g * PV_BINS;
  float2* out = a.phi + g * PV_BINS;
#pragma unroll
  for (int j = 0; j < 17; ++j) {
    const int b = 64 * j + lane;
    if (b >= PV_BINS) continue;
    float2 r = psi[b];
    if (!single) {
      const float2 uc = u[b], m = um[b];
      const double2 d = pv_mul64(make_double2((double)uc.x, (double)uc.y), make_double2((double)m.x, -(double)m.y));
      const double2 q = pv_ph64(pv_mul64(make_double2((double)r.x, (double)r.y), d));
      r = make_float2((float)q.x, (float)q.y);
    }
    out[b] = r;
  }
}

int launch_pv_rotate(Context& ctx, const float2* psi, const float2* u_mid, const int64_t* mid_base, const float2* u,
                     const int64_t* frame_base, const int* group_first, int n_files, int n_groups,
                     int64_t total_frames, float2* phi, hipStream_t st) {
  if (n_files < 0 || n_files > 65535 || n_groups < 0 || n_groups > n_files || total_frames < 0 ||
      (total_frames + 3) / 4 > 0x7fffffff) {
    set_error("pv_rotate: need 0 .. 65535 files, at most as many groups and total_frames >= 0");
    return -2;
  }
  if (n_files == 0 || total_frames == 0) return 0;
  if (n_groups == 0 || !psi || !u_mid || !mid_base || !u || !frame_base || !group_first || !phi) {
    set_error("pv_rotate: null argument");
    return -2;
  }
  PvRotArgs a{psi, u_mid, mid_base, u, frame_base, group_first, n_files, n_groups, total_frames, phi, nullptr};
  {
    KTimer kt_(ctx, "pv_rotate", st);
    a.span = kt_.span();
    hipLaunchKernelGGL(pv_rotate_kernel, dim3((unsigned)((total_frames + 3) / 4)), dim3(256), 0, st, a);
  }
  NC_HIP(hipGetLastError());
  return 0;
}

// nc_pv_stretch: analysis, scan and synthesis on one workspace laid out by the caller (ws_off,
// as pv_plan returns it or roomier)
int launch_pv_stretch(Context& ctx, const float* x, const int64_t* in_off, const int64_t* in_len,
                      const int64_t* frame_base, int n_files, int64_t total_frames, int64_t max_frames, int64_t P,
                      int64_t max_ns, float* s, const int64_t* out_off, float* peak, void* ws, const int64_t* ws_off,
                      size_t ws_bytes, hipStream_t st) {
  if (n_files < 0 || total_frames < 0) {
    set_error("nc_pv_stretch: negative file or frame count");
    return -2;
  }
  size_t need[6];
  pv_stretch_sizes(total_frames, std::max(0, n_files), need);
  if (total_frames > 0) {
    if (!ws || !ws_off) {
      set_error("nc_pv_stretch: null workspace");
      return -2;
    }
    for (int i = 0; i < 6; ++i) {
      const int64_t end = i + 1 < 6 ? ws_off[i + 1] : (int64_t)ws_bytes;
      if (ws_off[i] < 0 || (ws_off[i] & 15) || end < ws_off[i] || (size_t)(end - ws_off[i]) < need[i] ||
          (size_t)end > ws_bytes) {
        set_error("nc_pv_stretch: workspace below nc_pv_plan's layout");
        return -2;
      }
    }
  }
  auto sec = [&](int i) { return total_frames > 0 ? static_cast<char*>(ws) + ws_off[i] : nullptr; };
  float* mag = reinterpret_cast<float*>(sec(0));
  float2 *v = reinterpret_cast<float2*>(sec(1)), *phi = reinterpret_cast<float2*>(sec(2));
  float* frames = reinterpret_cast<float*>(sec(3));
  uint8_t* empty = reinterpret_cast<uint8_t*>(sec(4));
  int rc = launch_pv_analyze(ctx, x, in_off, in_len, frame_base, n_files, total_frames, P, mag, v, empty, nullptr,
                             false, st);
  if (rc) return rc;
  rc = launch_pv_scan(ctx, v, empty, frame_base, n_files, total_frames, max_frames, phi, sec(5),
                      total_frames > 0 ? ws_bytes - (size_t)ws_off[5] : 0, st);
  if (rc) return rc;
  return launch_pv_synth(ctx, mag, phi, in_len, frame_base, n_files, total_frames, P, max_ns, frames, need[3], s,
                         out_off, peak, st);
}

}  // namespace nc
