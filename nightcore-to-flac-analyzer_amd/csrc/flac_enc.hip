// flac_enc.hip — FLAC frame encode on the device (nc_flac_encode / nc_flac_pack in include/ncgpu.h).
// One workgroup of one wave per frame, fixed block size streams:
//
//   A  all lanes: float32 input is quantised to the int32 work buffer (clamps counted), int32
//      input is checked against the sample size.
//   B  per signal (a channel; for two channels also mid and side) the choice rule of DESIGN.md §4
//      "FLAC encode": CONSTANT, VERBATIM, FIXED 0-4 and, at level 1, LPC 1-8, each predictor with
//      the exact Rice search: lanes tally sum(u >> k) for every k over the finest partition order
//      and an xor butterfly merges the tallies upward, one partition order per step.
//   C  the channel assignment, the frame's length, the slot's words zeroed.
//   D  lane 0 writes the header; per subframe each lane owns a contiguous run of samples, a wave
//      prefix sum of the runs' bit lengths gives its bit offset, it stores the words it fully owns
//      and ORs the boundary words atomically into the zeroed slot (big-endian bit order).
//   E  CRC-16 by the whole wave (nc_flac_crc.h), the footer, the frame's record.
//
// Safety (a bad table row gives a status, never an access):
//   - the frame's and the file's rows are checked against each other and against the buffer
//     lengths before anything is read or stored through them;
//   - samples are read only at x[c stride + i], 0 <= i < block (first + block <= total <= stride);
//   - every word store / atomic OR goes through Writer::flush, which drops words outside the slot;
//     the slot is sized by the VERBATIM bound, which the choice rule never exceeds;
//   - all loops are bounded by the block size, the channel count, the order or the partitions;
//     a unary run is bounded by the frame's length (a subframe is never longer than VERBATIM).
// The byte buffers are accessed as aligned 32-bit words only (Writer::flush, the CRC's loads, the
// pack kernel); LDS holds ints and naturally aligned 64-bit values behind address-space-known
// pointers, so the compiler emits ds_ instructions for it and no flat access.
#ifndef NC_FLAC_HOST_SIM
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "nc_launch.h"
#define NC_COHERENT_LOAD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#endif
#include "nc_flac_crc.h"

namespace nc {
namespace {

constexpr int FE_OK = 0, FE_ROW = 1, FE_RANGE = 2;
constexpr int FE_MAXCH = 8, FE_REC = 1 + 3 * FE_MAXCH;
constexpr int ST_CONST = 0, ST_VERBATIM = 1, ST_FIXED = 2, ST_LPC = 3;
constexpr int KIND_MID = 8, KIND_SIDE = 9;
constexpr int LPC_MAX = 8;

struct Src {
  const int* x;  // channel c's samples of this frame: x[c stride + i], i < block
  int64_t stride;
};

__device__ inline int sig_at(const Src& s, int kind, int i) {
  if (kind < FE_MAXCH) return s.x[kind * s.stride + i];
  const int l = s.x[i], r = s.x[s.stride + i];
  return kind == KIND_MID ? (l + r) >> 1 : l - r;
}

__device__ inline uint64_t shfl_xor64(uint64_t v, int d) {
#ifdef NC_FLAC_HOST_SIM
  return __shfl_xor(v, d, 64);  // one exchange instead of two
#endif
  const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d, 64), hi = (uint32_t)__shfl_xor((int)(v >> 32), d, 64);
  return ((uint64_t)hi << 32) | lo;
}
__device__ inline uint64_t wave_sum64(uint64_t v) {
  for (int d = 1; d < 64; d <<= 1) v += shfl_xor64(v, d);
  return v;
}
__device__ inline int wave_or(int v) {
  for (int d = 1; d < 64; d <<= 1) v |= __shfl_xor(v, d, 64);
  return v;
}

struct Best {  // uniform over the wave
  int type, order, po, shift, prec;
  uint64_t bits;
};

// residual of sample i (>= order) under the predictor cf / shift (FIXED: binomials, shift 0)
template <int M>
__device__ inline int64_t residual_at(const Src& s, int kind, int i, int order, const int (&cf)[M], int shift) {
  int64_t acc = 0;
#pragma unroll
  for (int j = 0; j < M; ++j)
    if (j < order) acc += (int64_t)cf[j] * (int64_t)sig_at(s, kind, i - 1 - j);
  return (int64_t)sig_at(s, kind, i) - (acc >> shift);
}

__device__ inline uint32_t fold(int e) { return ((uint32_t)e << 1) ^ (uint32_t)(e >> 31); }

// One predictor against the running best: the exact Rice cost for every partition order.
// NK = 15 (method 0, k <= 14) or 31 (method 1, k <= 30).  ks / coefs: the slot's LDS arrays.
template <int M, int NK>
__device__ void search(const Src& s, int kind, int block, int w, int type, int order, const int (&cf)[M], int shift,
                       int prec, Best& best, int* ks, int* coefs, int lane) {
  if (order >= block) return;
  int P = 0;
  while (P < 6 && (block & ((2 << P) - 1)) == 0 && (block >> (P + 1)) > order) ++P;
  const int lpp = 64 >> P, psize = block >> P;  // lanes per finest partition, its samples
  const int part = lane >> (6 - P), j0 = lane & (lpp - 1);
  uint64_t sum[NK];
#pragma unroll
  for (int k = 0; k < NK; ++k) sum[k] = 0;
  int bad = 0;
  for (int t = j0; t < psize; t += lpp) {
    const int i = part * psize + t;
    if (i < order) continue;
    const int64_t e64 = residual_at<M>(s, kind, i, order, cf, shift);
    if (e64 < -INT64_C(2147483648) || e64 > INT64_C(2147483647)) {
      bad = 1;
      continue;
    }
    const uint32_t u = fold((int)e64);
#pragma unroll
    for (int k = 0; k < NK; ++k) sum[k] += u >> k;
  }
  if (wave_or(bad)) return;  // a residual outside int32: the candidate is dropped
  const int pbits = NK == 15 ? 4 : 5;
  const uint64_t head = 8 + (uint64_t)order * w + (type == ST_LPC ? 9 + order * prec : 0) + 6;
  int kk[7];
  uint64_t lbits = ~UINT64_C(0);
  int lidx = -1;
#pragma unroll
  for (int lv = 0; lv < 7; ++lv) {  // groups of D = 2^lv lanes hold one partition's sums: order 6 - lv
    const int D = 1 << lv;
    kk[lv] = 0;
    if (D >= lpp) {
      const int po = 6 - lv;
      const uint64_t n = (uint64_t)((block >> po) - ((lane >> lv) == 0 ? order : 0));
      uint64_t bb = ~UINT64_C(0);
      int kb = 0;
#pragma unroll
      for (int k = 0; k < NK; ++k) {
        const uint64_t c = n * (k + 1) + sum[k];
        if (c < bb) {
          bb = c;
          kb = k;
        }
      }
      kk[lv] = kb;
      const uint64_t cost = head + wave_sum64((lane & (D - 1)) == 0 ? bb + pbits : 0);
      if (cost <= lbits) {  // a tie goes to the smaller partition order
        lbits = cost;
        lidx = lv;
      }
    }
    if (lv < 6) {
#pragma unroll
      for (int k = 0; k < NK; ++k) sum[k] += shfl_xor64(sum[k], D);
    }
  }
  if (lidx >= 0 && lbits < best.bits) {  // a tie goes to the earlier candidate
    best.type = type;
    best.order = order;
    best.po = 6 - lidx;
    best.shift = shift;
    best.prec = prec;
    best.bits = lbits;
    int k = 0;
#pragma unroll
    for (int lv = 0; lv < 7; ++lv)
      if (lv == lidx) k = kk[lv];
    if ((lane & ((1 << lidx) - 1)) == 0) ks[lane >> lidx] = k;
#pragma unroll
    for (int j = 0; j < M; ++j)
      if (lane == j) coefs[j] = cf[j];
  }
  __syncthreads();
}

// Level 1: Hann window, autocorrelation r[0 .. 8] in float64 by all lanes, Levinson-Durbin and the
// quantisation of every order's coefficients in lane 0.  lpc[o - 1][0 .. o) / lshift[o - 1]
// (-1: no candidate of this order) in LDS.
__device__ void lpc_analyse(const Src& s, int kind, int block, int prec, double* racc, int (*lpc)[LPC_MAX], int* lshift,
                            int lane) {
  const int per = (block + 63) / 64;
  const int i0 = lane * per, i1 = i0 + per < block ? i0 + per : block;
  const float step = block > 1 ? 6.28318530717958647692f / (float)(block - 1) : 0.0f;
  double r[LPC_MAX + 1], h[LPC_MAX + 1];
#pragma unroll
  for (int j = 0; j <= LPC_MAX; ++j) r[j] = h[j] = 0.0;
  for (int i = i0 - LPC_MAX; i < i1; ++i) {
    const double a = i >= 0 ? (double)(0.5f - 0.5f * cosf(step * (float)i)) * (double)sig_at(s, kind, i) : 0.0;
#pragma unroll
    for (int j = LPC_MAX; j > 0; --j) h[j] = h[j - 1];
    h[0] = a;
    if (i >= i0) {
#pragma unroll
      for (int j = 0; j <= LPC_MAX; ++j) r[j] += a * h[j];
    }
  }
#pragma unroll
  for (int j = 0; j <= LPC_MAX; ++j) {
    uint64_t bits;
    for (int d = 1; d < 64; d <<= 1) {
      __builtin_memcpy(&bits, &r[j], 8);
      bits = shfl_xor64(bits, d);
      double o;
      __builtin_memcpy(&o, &bits, 8);
      r[j] += o;
    }
    if (lane == 0) racc[j] = r[j];
  }
  if (lane < LPC_MAX) lshift[lane] = -1;
  __syncthreads();
  if (lane == 0 && racc[0] > 0.0) {
    double a[LPC_MAX], err = racc[0];
    const int qmax = (1 << (prec - 1)) - 1, qmin = -(1 << (prec - 1));
    for (int i = 0; i < LPC_MAX; ++i) {
      double acc = racc[i + 1];
      for (int j = 0; j < i; ++j) acc -= a[j] * racc[i - j];
      const double k = acc / err;
      if (!(k > -1.0 && k < 1.0)) break;
      for (int j = 0; j < i / 2; ++j) {
        const double t = a[j];
        a[j] = t - k * a[i - 1 - j];
        a[i - 1 - j] -= k * t;
      }
      if (i & 1) a[i / 2] -= k * a[i / 2];
      a[i] = k;
      err *= 1.0 - k * k;
      double cmax = 0.0;
      for (int j = 0; j <= i; ++j) cmax = fmax(cmax, fabs(a[j]));
      if (cmax > 0.0) {
        int e;
        frexp(cmax, &e);
        int sh = prec - 1 - e;
        if (sh > 15) sh = 15;
        if (sh >= 0) {
          double fb = 0.0;
          for (int j = 0; j <= i; ++j) {
            fb += ldexp(a[j], sh);
            double q = rint(fb);
            if (q > qmax) q = qmax;
            if (q < qmin) q = qmin;
            lpc[i][j] = (int)q;
            fb -= q;
          }
          lshift[i] = sh;
        }
      }
      if (!(err > 0.0)) break;
    }
  }
  __syncthreads();
}

struct LpcLds {
  double racc[LPC_MAX + 1];
  int coef[LPC_MAX][LPC_MAX];
  int shift[LPC_MAX];
};

// the choice rule for one signal of width w; ks / coefs: the slot's LDS arrays
template <int NK>
__device__ Best evaluate(const Src& s, int kind, int block, int w, int level, int prec, int* ks, int* coefs, LpcLds* ll,
                         int lane) {
  const int x0 = sig_at(s, kind, 0);
  int diff = 0;
  for (int i = lane; i < block; i += 64) diff |= sig_at(s, kind, i) != x0;
  const bool constant = !wave_or(diff);
  const uint64_t vb = 8 + (uint64_t)block * w;
  Best best = {ST_VERBATIM, 0, 0, 0, 0, vb + 1};  // FIXED wins a tie with VERBATIM
  const int omax = block - 1 < 4 ? block - 1 : 4;
  for (int o = 0; o <= omax; ++o) {
    const int fixed[5][4] = {{0, 0, 0, 0}, {1, 0, 0, 0}, {2, -1, 0, 0}, {3, -3, 1, 0}, {4, -6, 4, -1}};
    const int cf[4] = {fixed[o][0], fixed[o][1], fixed[o][2], fixed[o][3]};
    search<4, NK>(s, kind, block, w, ST_FIXED, o, cf, 0, 0, best, ks, coefs, lane);
  }
  if (best.type == ST_VERBATIM) best.bits = vb;
  if (constant && (uint64_t)(8 + w) <= best.bits) {
    best = Best{ST_CONST, 0, 0, 0, 0, (uint64_t)(8 + w)};
  }
  if (level >= 1 && !constant) {
    lpc_analyse(s, kind, block, prec, ll->racc, ll->coef, ll->shift, lane);
    for (int o = 1; o <= LPC_MAX; ++o) {
      const int sh = ll->shift[o - 1];
      if (sh < 0) continue;
      int cf[LPC_MAX];
#pragma unroll
      for (int j = 0; j < LPC_MAX; ++j) cf[j] = j < o ? ll->coef[o - 1][j] : 0;
      search<LPC_MAX, NK>(s, kind, block, w, ST_LPC, o, cf, sh, prec, best, ks, coefs, lane);
    }
  }
  return best;
}

struct Counter {
  uint32_t n;
  __device__ void put(uint32_t, int nb) { n += nb; }
  __device__ void unary(uint32_t q) { n += q + 1; }
};

struct Writer {
  uint32_t* words;   // the frame's slot
  uint32_t n_words;  // its length
  uint32_t pos;      // bit offset of the word being filled
  uint64_t acc;      // its bits so far, then nothing
  int fill;          // 0 .. 31
  bool shared, all_atomic;

  __device__ void init(uint32_t* w, uint32_t nw, uint32_t bit, bool atomics) {
    words = w;
    n_words = nw;
    pos = bit & ~31u;
    fill = (int)(bit & 31u);
    acc = 0;
    all_atomic = atomics;
    shared = atomics || fill != 0;
  }
  __device__ void flush(uint32_t v) {
    const uint32_t wi = pos >> 5;
    if (wi < n_words) {
      if (shared) atomicOr(words + wi, __builtin_bswap32(v));
      else words[wi] = __builtin_bswap32(v);
    }
    pos += 32;
    shared = all_atomic;
  }
  __device__ void put(uint32_t v, int nb) {  // 0 <= nb <= 32, v < 2^nb
    if (nb == 0) return;
    acc = (acc << nb) | v;
    fill += nb;
    if (fill >= 32) {
      fill -= 32;
      flush((uint32_t)(acc >> fill));
      acc &= (UINT64_C(1) << fill) - 1;
    }
  }
  __device__ void unary(uint32_t q) {  // q zeros and a one; runs of any length
    while (q >= 32) {
      put(0, 32);
      q -= 32;
    }
    put(1, (int)q + 1);
  }
  __device__ void finish() {
    if (fill) {
      shared = true;
      flush((uint32_t)(acc << (32 - fill)));
      fill = 0;
      acc = 0;
    }
  }
};

// the bits of samples [i0, i1) of one subframe (the subframe's header goes with sample 0, the
// predictor's fields and the residual header with sample `order`)
template <class Sink>
__device__ void emit_sub(Sink& o, const Src& s, int kind, int block, int w, const Best& b, int method, const int* ks,
                         const int (&cf)[LPC_MAX], int i0, int i1) {
  const uint32_t mask = (1u << w) - 1;
  if (i0 == 0 && i1 > 0) {
    const int code = b.type == ST_CONST ? 0 : b.type == ST_VERBATIM ? 1 : b.type == ST_FIXED ? 8 + b.order : 31 + b.order;
    o.put((uint32_t)code << 1, 8);
    if (b.type == ST_CONST) o.put((uint32_t)sig_at(s, kind, 0) & mask, w);
  }
  if (b.type == ST_CONST) return;
  if (b.type == ST_VERBATIM) {
    for (int i = i0; i < i1; ++i) o.put((uint32_t)sig_at(s, kind, i) & mask, w);
    return;
  }
  const int psz = block >> b.po, pbits = 4 + method;
  for (int i = i0; i < i1; ++i) {
    if (i < b.order) {
      o.put((uint32_t)sig_at(s, kind, i) & mask, w);
      continue;
    }
    if (i == b.order) {
      if (b.type == ST_LPC) {
        o.put((uint32_t)(b.prec - 1), 4);
        o.put((uint32_t)b.shift & 31u, 5);
#pragma unroll
        for (int j = 0; j < LPC_MAX; ++j)
          if (j < b.order) o.put((uint32_t)cf[j] & ((1u << b.prec) - 1), b.prec);
      }
      o.put((uint32_t)method, 2);
      o.put((uint32_t)b.po, 4);
    }
    const int part = i / psz;
    const int k = ks[part & 63];
    if (i == b.order || i == part * psz) o.put((uint32_t)k, pbits);
    const uint32_t u = fold((int)residual_at<LPC_MAX>(s, kind, i, b.order, cf, b.shift));
    o.unary(u >> k);
    o.put(u & ((1u << k) - 1), k);
  }
}

__device__ inline int utf8_extra(uint32_t v) {  // continuation bytes of the coded number
  int n = 0;
  if (v >= 0x80) {
    n = 1;
    while (n < 6 && v >= (1u << (5 * n + 6))) ++n;
  }
  return n;
}

__device__ inline int block_code(int block) {
  if (block == 192) return 1;
  for (int c = 2; c < 6; ++c)
    if (block == 576 << (c - 2)) return c;
  for (int c = 8; c < 16; ++c)
    if (block == 256 << (c - 8)) return c;
  return block <= 256 ? 6 : 7;
}

__device__ inline int rate_code(int64_t rate) {
  const int table[11] = {88200, 176400, 192000, 8000, 16000, 22050, 24000, 32000, 44100, 48000, 96000};
  for (int i = 0; i < 11; ++i)
    if (rate == table[i]) return i + 1;
  return 0;
}

__device__ inline int bits_code(int bits) {
  return bits == 8 ? 1 : bits == 12 ? 2 : bits == 16 ? 4 : bits == 20 ? 5 : bits == 24 ? 6 : 0;
}

struct SlotLds {
  int ks[64];
  int coef[LPC_MAX];
};

__device__ inline uint32_t slot_need(int nch, int block, int bits) {  // the VERBATIM bound, bytes
  const uint32_t body = (uint32_t)nch * (8u + (uint32_t)block * (uint32_t)(bits + 1));
  return (16u + ((body + 7u) >> 3) + 2u + 3u) & ~3u;
}

// files: int64 [n_files][8] = in_off, channel stride, channels, bits per sample, rate, total
// samples, 0, 0.  frames: int64 [n_frames][8] = file, first sample, block, frame number, slot
// offset (bytes, a multiple of 4), 0, 0, 0.
__global__ __launch_bounds__(64) void flac_encode_kernel(const int* pcm_in, const float* f32_in,
                                                         int* pcm_q, int64_t in_len, const int64_t* __restrict__ frames,
                                                         int64_t n_frames, const int64_t* __restrict__ files,
                                                         int n_files, int level, uint32_t* slots, int64_t slot_bytes,
                                                         int* __restrict__ frame_bytes, int* __restrict__ records,
                                                         int* __restrict__ clipped, int* __restrict__ status) {
  __shared__ SlotLds slot[FE_MAXCH];
  __shared__ LpcLds ll;
  __shared__ Best best[FE_MAXCH];
  __shared__ uint32_t crc_tab[256];
  const int lane = threadIdx.x;
  const int64_t fr = blockIdx.x;
  if (fr >= n_frames) return;
  const int64_t* row = frames + 8 * fr;
  const int64_t file = row[0], first = row[1], block64 = row[2], number = row[3], slot_off = row[4];
  bool ok = file >= 0 && file < n_files && first >= 0 && block64 >= 1 && block64 <= 16384 && number >= 0 &&
            number < (INT64_C(1) << 31) && slot_off >= 0 && (slot_off & 3) == 0 && slot_bytes >= 0 && in_len >= 0;
  int64_t in_off = 0, stride = 0, rate = 0;
  int nch = 0, bits = 0;
  if (ok) {
    const int64_t* fl = files + 8 * file;
    in_off = fl[0];
    stride = fl[1];
    nch = (int)(fl[2] >= 1 && fl[2] <= FE_MAXCH ? fl[2] : 0);
    bits = (int)(fl[3] >= 4 && fl[3] <= 24 ? fl[3] : 0);
    rate = fl[4];
    const int64_t total = fl[5];
    ok = nch > 0 && bits > 0 && rate >= 0 && rate < (INT64_C(1) << 20) && total >= 0 && total <= (INT64_C(1) << 36) &&
         first <= total - block64 && stride >= total && stride <= in_len && in_off >= 0 &&
         in_off <= in_len - (int64_t)nch * stride;
    if (ok) ok = slot_off <= slot_bytes - (int64_t)slot_need(nch, (int)block64, bits);
  }
  if (!ok) {
    if (lane == 0) {
      status[fr] = FE_ROW;
      frame_bytes[fr] = 0;
      clipped[fr] = 0;
    }
    return;
  }
  const int block = (int)block64;
  const int64_t base = in_off + first;

  // A: the frame's samples as int32
  const int lo = -(1 << (bits - 1)), hi = (1 << (bits - 1)) - 1;
  int cnt = 0, out_of_range = 0;
  if (f32_in) {
    const float scale = (float)(1 << (bits - 1)), flo = (float)lo, fhi = (float)hi;
    for (int c = 0; c < nch; ++c)
      for (int i = lane; i < block; i += 64) {
        const float v = rintf(f32_in[base + c * stride + i] * scale);
        cnt += (v > fhi || v < flo) ? 1 : 0;
        pcm_q[base + c * stride + i] = (int)fminf(fmaxf(v, flo), fhi);
      }
    __threadfence();
    __syncthreads();
  } else {
    for (int c = 0; c < nch; ++c)
      for (int i = lane; i < block; i += 64) {
        const int v = pcm_in[base + c * stride + i];
        out_of_range |= (v < lo || v > hi) ? 1 : 0;
        if (pcm_q) pcm_q[base + c * stride + i] = v;
      }
  }
  cnt = (int)wave_sum64((uint64_t)cnt);
  if (wave_or(out_of_range)) {
    if (lane == 0) {
      status[fr] = FE_RANGE;
      frame_bytes[fr] = 0;
      clipped[fr] = 0;
    }
    return;
  }
  Src s;
  s.x = (f32_in ? pcm_q : pcm_in) + base;
  s.stride = stride;

  // B: the choice per signal
  const int method = bits > 16 ? 1 : 0, prec = bits > 16 ? 15 : 12;
  const int n_sig = nch == 2 ? 4 : nch;
#pragma unroll 1
  for (int g = 0; g < n_sig; ++g) {
    const int kind = nch == 2 && g >= 2 ? KIND_MID + (g - 2) : g, w = bits + (nch == 2 && g == 3 ? 1 : 0);
    Best b;
    if (method) b = evaluate<31>(s, kind, block, w, level, prec, slot[g].ks, slot[g].coef, &ll, lane);
    else b = evaluate<15>(s, kind, block, w, level, prec, slot[g].ks, slot[g].coef, &ll, lane);
    if (lane == 0) best[g] = b;
  }
  __syncthreads();

  // C: the assignment (ties: 1, 8, 9, 10), the frame's length
  int assign = nch - 1;
  int sub0 = 0, sub1 = 1;
  if (nch == 2) {
    const uint64_t a1 = best[0].bits + best[1].bits, a8 = best[0].bits + best[3].bits,
                   a9 = best[3].bits + best[1].bits, a10 = best[2].bits + best[3].bits;
    uint64_t m = a1;
    assign = 1;
    if (a8 < m) m = a8, assign = 8;
    if (a9 < m) m = a9, assign = 9;
    if (a10 < m) m = a10, assign = 10;
    if (assign == 8) sub1 = 3;
    if (assign == 9) sub0 = 3;
    if (assign == 10) sub0 = 2, sub1 = 3;
  }
  const int bs_code = block_code(block);
  const int hdr_len = 4 + 1 + utf8_extra((uint32_t)number) + (bs_code == 6 ? 1 : bs_code == 7 ? 2 : 0) + 1;
  uint64_t body_bits = 0;
  for (int c = 0; c < nch; ++c) body_bits += best[c == 0 ? sub0 : c == 1 ? sub1 : c].bits;
  const uint32_t need = slot_need(nch, block, bits);
  const uint64_t foot64 = (uint64_t)hdr_len + ((body_bits + 7) >> 3);
  if (foot64 + 2 > need) {  // cannot happen: every subframe costs at most VERBATIM
    if (lane == 0) {
      status[fr] = FE_RANGE;
      frame_bytes[fr] = 0;
      clipped[fr] = 0;
    }
    return;
  }
  const uint32_t foot = (uint32_t)foot64, n_words = need >> 2;
  uint32_t* words = slots + (slot_off >> 2);
  for (uint32_t i = lane; i < (foot + 2 + 3) >> 2; i += 64) words[i] = 0;
  crc16_fill_table(crc_tab, lane);
  __threadfence();
  __syncthreads();

  // D: header, subframes
  if (lane == 0) {
    Writer wr;
    wr.init(words, n_words, 0, true);
    uint32_t crc = 0;
    auto hput = [&](uint32_t b) {
      wr.put(b & 0xff, 8);
      crc ^= b & 0xff;
      for (int k = 0; k < 8; ++k) crc = ((crc << 1) ^ ((crc & 0x80) ? 0x07u : 0u)) & 0xff;
    };
    hput(0xFF);
    hput(0xF8);
    hput((uint32_t)(bs_code << 4) | (uint32_t)rate_code(rate));
    hput((uint32_t)(assign << 4) | (uint32_t)(bits_code(bits) << 1));
    const uint32_t v = (uint32_t)number;
    const int ex = utf8_extra(v);
    if (ex == 0) {
      hput(v);
    } else {
      hput(((0xFFu << (7 - ex)) & 0xFF) | (v >> (6 * ex)));
      for (int i = ex - 1; i >= 0; --i) hput(0x80 | ((v >> (6 * i)) & 0x3F));
    }
    if (bs_code == 6) hput((uint32_t)(block - 1));
    if (bs_code == 7) {
      hput((uint32_t)(block - 1) >> 8);
      hput((uint32_t)(block - 1));
    }
    hput(crc);
    wr.finish();
  }
  const int per = (block + 63) / 64;
  const int i0 = lane * per < block ? lane * per : block, i1 = i0 + per < block ? i0 + per : block;
  uint32_t bit = (uint32_t)hdr_len * 8;
  for (int c = 0; c < nch; ++c) {
    const int g_sel = c == 0 ? sub0 : c == 1 ? sub1 : c;
    const Best b = best[g_sel];
    const int kind = nch == 2 && g_sel >= 2 ? KIND_MID + (g_sel - 2) : g_sel, w = bits + (nch == 2 && g_sel == 3 ? 1 : 0);
    const int* ks = slot[g_sel].ks;
    int cf[LPC_MAX];
#pragma unroll
    for (int j = 0; j < LPC_MAX; ++j) cf[j] = (b.type == ST_FIXED || b.type == ST_LPC) && j < b.order ? slot[g_sel].coef[j] : 0;
    Counter cn;
    cn.n = 0;
    emit_sub(cn, s, kind, block, w, b, method, ks, cf, i0, i1);
    uint32_t incl = cn.n;
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t up = (uint32_t)__shfl_up((int)incl, d, 64);
      if (lane >= d) incl += up;
    }
    Writer wr;
    wr.init(words, n_words, bit + incl - cn.n, false);
    emit_sub(wr, s, kind, block, w, b, method, ks, cf, i0, i1);
    wr.finish();
    bit += (uint32_t)b.bits;
    if (lane == 0) {
      int* rec = records + FE_REC * fr + 1 + 3 * c;
      rec[0] = b.type;
      rec[1] = b.order;
      rec[2] = b.type >= ST_FIXED ? b.po : 0;
    }
  }
  __threadfence();
  __syncthreads();

  // E: CRC-16 of the bytes before the footer, the footer
  const uint32_t crc = wave_crc16(
      [words](int64_t g) { return (NC_COHERENT_LOAD(words + (g >> 2)) >> (8 * (uint32_t)(g & 3))) & 0xffu; }, foot,
      crc_tab, lane);
  if (lane == 0) {
    Writer wr;
    wr.init(words, n_words, foot * 8, true);
    wr.put(crc & 0xffff, 16);
    wr.finish();
    records[FE_REC * fr] = assign;
    for (int c = nch; c < FE_MAXCH; ++c) {
      int* rec = records + FE_REC * fr + 1 + 3 * c;
      rec[0] = rec[1] = rec[2] = 0;
    }
    frame_bytes[fr] = (int)(foot + 2);
    clipped[fr] = cnt;
    status[fr] = FE_OK;
  }
}

// frame fr's bytes slots[slot_off .. + frame_bytes[fr]) to out[offsets[fr] ..): aligned words of
// out, the boundary words OR-ed into the zeroed buffer
__global__ __launch_bounds__(64) void flac_pack_kernel(const uint32_t* __restrict__ slots, int64_t slot_bytes,
                                                       const int64_t* __restrict__ frames, int64_t n_frames,
                                                       const int* __restrict__ frame_bytes,
                                                       const int64_t* __restrict__ offsets, uint32_t* out,
                                                       int64_t out_bytes) {
  const int64_t fr = blockIdx.x;
  if (fr >= n_frames) return;
  const int64_t slot_off = frames[8 * fr + 4], len = frame_bytes[fr], off = offsets[fr];
  if (len <= 0 || slot_off < 0 || (slot_off & 3) || slot_off > slot_bytes - ((len + 3) & ~INT64_C(3)) || off < 0 ||
      off > out_bytes - len)
    return;
  const uint32_t* src = slots + (slot_off >> 2);
  const int64_t w0 = off >> 2, w1 = (off + len + 3) >> 2;  // w1 4 <= out_bytes (a multiple of 4)
  for (int64_t wi = w0 + threadIdx.x; wi < w1; wi += 64) {
    uint32_t v = 0;
    bool whole = true;
    for (int b = 0; b < 4; ++b) {
      const int64_t g = wi * 4 + b - off;
      if (g >= 0 && g < len) v |= ((src[g >> 2] >> (8 * (uint32_t)(g & 3))) & 0xffu) << (8 * b);
      else whole = false;
    }
    if (whole) out[wi] = v;
    else atomicOr(out + wi, v);
  }
}

}  // namespace

#ifndef NC_FLAC_HOST_SIM
int launch_flac_encode(const int* pcm_in, const float* f32_in, int* pcm_q, int64_t in_len, const int64_t* frames,
                       int64_t n_frames, const int64_t* files, int n_files, int level, uint8_t* slots,
                       int64_t slot_bytes, int* frame_bytes, int* records, int* clipped, int* status, hipStream_t st) {
  if (n_frames == 0) return 0;
  if (n_frames < 0 || n_frames > 0x7fffffff || n_files <= 0 || in_len < 0 || slot_bytes < 0 || level < 0 || level > 1) {
    set_error("flac_encode: need 0 .. 2^31-1 frames, at least one file and level 0 or 1");
    return -2;
  }
  if (!frames || !files || !slots || !frame_bytes || !records || !clipped || !status) {
    set_error("flac_encode: null argument");
    return -2;
  }
  if ((pcm_in != nullptr) == (f32_in != nullptr) || (f32_in && !pcm_q)) {
    set_error("flac_encode: give int32 samples, or float32 samples and the int32 buffer they are quantised into");
    return -2;
  }
  if ((reinterpret_cast<uintptr_t>(slots) & 3) || (slot_bytes & 3)) {
    set_error("flac_encode: the slot buffer must be 4-byte aligned and a multiple of 4 bytes long");
    return -2;
  }
  hipLaunchKernelGGL(flac_encode_kernel, dim3((unsigned)n_frames), dim3(64), 0, st, pcm_in, f32_in, pcm_q, in_len, frames,
                     n_frames, files, n_files, level, reinterpret_cast<uint32_t*>(slots), slot_bytes, frame_bytes,
                     records, clipped, status);
  NC_HIP(hipGetLastError());
  return 0;
}

int launch_flac_pack(const uint8_t* slots, int64_t slot_bytes, const int64_t* frames, int64_t n_frames,
                     const int* frame_bytes, const int64_t* offsets, uint8_t* out, int64_t out_bytes, hipStream_t st) {
  if (n_frames < 0 || n_frames > 0x7fffffff || slot_bytes < 0 || out_bytes < 0) {
    set_error("flac_pack: need 0 .. 2^31-1 frames and buffer lengths >= 0");
    return -2;
  }
  if (!out || (n_frames && (!slots || !frames || !frame_bytes || !offsets))) {
    set_error("flac_pack: null argument");
    return -2;
  }
  if ((reinterpret_cast<uintptr_t>(slots) & 3) || (reinterpret_cast<uintptr_t>(out) & 3) || (slot_bytes & 3) ||
      (out_bytes & 3)) {
    set_error("flac_pack: both byte buffers must be 4-byte aligned and a multiple of 4 bytes long");
    return -2;
  }
  if (out_bytes) NC_HIP(hipMemsetAsync(out, 0, (size_t)out_bytes, st));
  if (n_frames == 0) return 0;
  hipLaunchKernelGGL(flac_pack_kernel, dim3((unsigned)n_frames), dim3(64), 0, st,
                     reinterpret_cast<const uint32_t*>(slots), slot_bytes, frames, n_frames, frame_bytes, offsets,
                     reinterpret_cast<uint32_t*>(out), out_bytes);
  NC_HIP(hipGetLastError());
  return 0;
}
#endif

}  // namespace nc
