// flac.hip — FLAC frame decode on the device (nc_flac_decode in include/ncgpu.h; the frame table
// comes from nc_flac_index.cpp).  One workgroup of one wave per frame:
//
//   A  lane 0 walks the frame's bitstream (the subframes follow each other bit by bit, so this
//      scan is serial by the format): subframe headers, warm-up samples and predictor
//      coefficients go to LDS, Rice / escape residuals to the frame's own slots of the int32
//      output; a VERBATIM subframe is only measured (its samples sit at fixed bit offsets).
//   B  all lanes: CRC-16 of the bytes before the footer — 64 equal chunks, joined by
//      crc(A || B) = crc(A) x^(8 |B|) + crc(B) in GF(2)[x] / (x^16 + x^15 + x^2 + 1).
//   C  all lanes fill CONSTANT and VERBATIM subframes.
//   D  one lane per predicted channel runs the recurrence s[n] = r[n] + (sum c_i s[n-1-i]) >> shift
//      with a 64-bit sum (FIXED orders are the same recurrence with binomial coefficients and
//      shift 0), history and coefficients in registers, samples staged through LDS in tiles of
//      64 so global traffic stays coalesced.
//   E  all lanes: wasted bits back in, stereo decorrelation, int32 / float32 / mono stores.
//
// Safety (a corrupt stream gives a status, never a fault):
//   - bits are read only by Bits::get / unary / peek inside [0, end_bit) of the frame; a read that
//     would cross end_bit consumes nothing, returns 0 and sets FL_OVERRUN; word loads are clamped
//     to the buffer (which the caller pads by 8 bytes);
//   - every loop is bounded by the header's block size (<= 65535), the channel count (<= 8), the
//     predictor order (<= 32) or the frame's length in bits;
//   - every store is to pcm/f32[out_off + c stride + first + i] or mono[mono_off + first + i] with
//     0 <= i < block, after the kernel has checked first + block <= total <= stride and the file's
//     row against the buffer lengths.
//
// The frame's bytes are read from global memory through aligned 32-bit words, two at a time (the
// compiler joins them into one 8-byte load at a 4-byte aligned address).  Keep them there: a copy
// of the frame in LDS read through the same generic pointer turns that into a misaligned 8-byte
// flat access to LDS, which the MI355X answers with a memory aperture violation.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nc_launch.h"
#include "nc_flac_crc.h"

namespace nc {
namespace {

constexpr int FL_OK = 0, FL_CRC = 1, FL_OVERRUN = 2, FL_INVALID = 3, FL_LENGTH = 4;
constexpr int FL_MAXCH = 8, FL_MAXORD = 32;
constexpr int T_CONST = 0, T_VERBATIM = 1, T_PREDICT = 2;

struct Sub {
  int type, order, shift, wasted, bps;
  int value;            // CONSTANT: the sample; VERBATIM: bit offset of the first sample
  int coef[FL_MAXORD];  // coef[i] multiplies s[n-1-i]
};

struct Bits {
  const uint32_t* words;  // the byte buffer as aligned big-endian words
  int64_t n_words;
  uint64_t base_bit;      // 8 * frame start
  uint32_t end_bit;       // 8 * frame length (<= 2^30)
  uint32_t pos;           // <= end_bit, always
  int err;

  // 32 bits from bit `at` (< end_bit); bits past the buffer's end never reach a caller
  __device__ uint32_t peek(uint32_t at) const {
    const uint64_t a = base_bit + at;
    int64_t w = (int64_t)(a >> 5);
    if (w > n_words - 2) w = n_words - 2;
    const uint64_t v = ((uint64_t)__builtin_bswap32(words[w]) << 32) | __builtin_bswap32(words[w + 1]);
    return (uint32_t)((v << (a & 31)) >> 32);
  }
  __device__ uint32_t get(int n) {  // 0 <= n <= 32
    if (n == 0) return 0;
    if (err || n > (int)(end_bit - pos)) {
      if (!err) err = FL_OVERRUN;
      return 0;
    }
    const uint32_t v = peek(pos) >> (32 - n);
    pos += n;
    return v;
  }
  __device__ int sget(int n) {
    if (n == 0) return 0;
    return (int)(get(n) << (32 - n)) >> (32 - n);
  }
  __device__ uint32_t unary() {  // zeros before the next 1, which is consumed; runs of any length
    uint32_t q = 0;
    while (true) {
      if (err) return 0;
      if (pos >= end_bit) {
        err = FL_OVERRUN;
        return 0;
      }
      const uint32_t avail = end_bit - pos;
      uint32_t w = peek(pos);
      if (avail < 32) w &= ~(0xffffffffu >> avail);
      if (w == 0) {
        const uint32_t step = avail < 32 ? avail : 32;
        q += step;
        pos += step;
        continue;
      }
      const uint32_t z = __clz(w);
      q += z;
      pos += z + 1;
      return q;
    }
  }
};

// residual of one subframe into out[order .. block)
__device__ void residual(Bits& b, int* out, int block, int order) {
  const int method = b.get(2);
  if (b.err) return;
  if (method > 1) {
    b.err = FL_INVALID;
    return;
  }
  const int pbits = 4 + method, esc = (1 << pbits) - 1;
  const int po = b.get(4);
  if (b.err) return;
  const int psize = block >> po;
  if ((psize << po) != block || psize < order) {
    b.err = FL_LENGTH;
    return;
  }
  int n = order;
  for (int p = 0; p < (1 << po); ++p) {
    const int cnt = psize - (p == 0 ? order : 0);
    const int k = b.get(pbits);
    if (b.err) return;
    if (k == esc) {
      const int nb = b.get(5);
      for (int j = 0; j < cnt; ++j) {
        out[n++] = b.sget(nb);
        if (b.err) return;
      }
    } else {
      for (int j = 0; j < cnt; ++j) {
        const uint32_t q = b.unary();
        const uint32_t u = (q << k) | b.get(k);
        if (b.err) return;
        out[n++] = (int)(u >> 1) ^ -(int)(u & 1);
      }
    }
  }
  if (n != block) b.err = FL_LENGTH;
}

// lane 0: the subframes of one frame; returns the byte offset of the CRC-16 footer
__device__ uint32_t parse_frame(Bits& b, Sub* sub, int* out0, int64_t stride, int nch, int block, int bps,
                                int assign) {
  for (int c = 0; c < nch; ++c) {
    Sub& s = sub[c];
    const int side = (assign == 8 && c == 1) || (assign == 9 && c == 0) || (assign == 10 && c == 1);
    int sb = bps + side;
    const uint32_t head = b.get(8);
    if (b.err) return 0;
    if (head & 0x80) {  // padding bit
      b.err = FL_INVALID;
      return 0;
    }
    const int t = (head >> 1) & 63;
    int wasted = 0;
    if (head & 1) wasted = (int)b.unary() + 1;
    if (b.err) return 0;
    if (wasted >= sb) {
      b.err = FL_INVALID;
      return 0;
    }
    sb -= wasted;
    s.wasted = wasted;
    s.bps = sb;
    s.order = 0;
    s.shift = 0;
    int* out = out0 + c * stride;
    if (t == 0) {
      s.type = T_CONST;
      s.value = b.sget(sb);
    } else if (t == 1) {
      s.type = T_VERBATIM;
      s.value = (int)b.pos;
      const uint32_t need = (uint32_t)block * (uint32_t)sb;  // <= 65535 * 25
      if (need > b.end_bit - b.pos) {
        b.err = FL_OVERRUN;
        return 0;
      }
      b.pos += need;
    } else if ((t & 0x38) == 0x08 || (t & 0x20)) {
      const bool lpc = (t & 0x20) != 0;
      const int order = lpc ? (t & 31) + 1 : (t & 7);
      if ((!lpc && order > 4) || order > block) {
        b.err = FL_INVALID;
        return 0;
      }
      s.type = T_PREDICT;
      s.order = order;
      for (int i = 0; i < order; ++i) out[i] = b.sget(sb);
      if (lpc) {
        const int prec = (int)b.get(4) + 1;
        const int shift = b.sget(5);
        if (b.err) return 0;
        if (prec == 16 || shift < 0) {
          b.err = FL_INVALID;
          return 0;
        }
        s.shift = shift;
        for (int i = 0; i < order; ++i) s.coef[i] = b.sget(prec);
      } else {
        const int fixed[5][4] = {{0, 0, 0, 0}, {1, 0, 0, 0}, {2, -1, 0, 0}, {3, -3, 1, 0}, {4, -6, 4, -1}};
        for (int i = 0; i < order; ++i) s.coef[i] = fixed[order][i];
      }
      if (b.err) return 0;
      residual(b, out, block, order);
    } else {
      b.err = FL_INVALID;  // reserved subframe type
    }
    if (b.err) return 0;
  }
  b.pos = (b.pos + 7) & ~7u;  // zero padding to the byte; end_bit is a multiple of 8
  if (b.end_bit - b.pos < 16) {
    b.err = FL_OVERRUN;
    return 0;
  }
  return b.pos >> 3;
}

// phase D for predictor orders up to M (history and coefficients in registers)
template <int M>
__device__ void restore(const Sub* sub, int (*tile)[64], int* out0, int64_t stride, int nch, int block, int lane) {
  const bool active = lane < nch && sub[lane < nch ? lane : 0].type == T_PREDICT;
  const Sub& s = sub[active ? lane : 0];
  const int order = active ? s.order : 0, shift = s.shift;
  int h[M], cf[M];
#pragma unroll
  for (int i = 0; i < M; ++i) {
    cf[i] = i < order ? s.coef[i] : 0;
    h[i] = 0;
  }
  for (int base = 0; base < block; base += 64) {
    const int n_here = block - base < 64 ? block - base : 64;
    for (int c = 0; c < nch; ++c)
      if (sub[c].type == T_PREDICT) tile[c][lane] = lane < n_here ? out0[c * stride + base + lane] : 0;
    __syncthreads();
    if (active) {
      for (int j = 0; j < n_here; ++j) {
        int r = tile[lane][j];
        if (base + j >= order) {
          int64_t acc = 0;
#pragma unroll
          for (int i = 0; i < M; ++i) acc += (int64_t)cf[i] * (int64_t)h[i];
          r = (int)((uint32_t)r + (uint32_t)(acc >> shift));
        }
#pragma unroll
        for (int i = M - 1; i > 0; --i) h[i] = h[i - 1];
        h[0] = r;
        tile[lane][j] = r;
      }
    }
    __syncthreads();
    for (int c = 0; c < nch; ++c)
      if (sub[c].type == T_PREDICT && lane < n_here) out0[c * stride + base + lane] = tile[c][lane];
  }
}

// frames: int64 [n_frames][8] = byte start, byte end, first sample, block size, channel
// assignment, bits per sample, header bytes, file.  files: int64 [n_files][8] = out_off,
// channel stride, channels, bits per sample, total samples, mono_off (-1: none), 0, 0.
__global__ __launch_bounds__(64) void flac_frame_kernel(const uint8_t* __restrict__ data, int64_t data_bytes,
                                                        const int64_t* __restrict__ frames, int64_t n_frames,
                                                        const int64_t* __restrict__ files, int n_files, int* pcm,
                                                        float* f32, int64_t pcm_len, float* mono, int64_t mono_len,
                                                        int* __restrict__ status) {
  __shared__ Sub sub[FL_MAXCH];
  __shared__ int tile[FL_MAXCH][64];
  __shared__ uint16_t crc_tab[256];
  __shared__ int s_err;
  __shared__ uint32_t s_foot;
  const int lane = threadIdx.x;
  const int64_t fr = blockIdx.x;
  if (fr >= n_frames) return;
  const int64_t* row = frames + 8 * fr;
  const int64_t start = row[0], end = row[1], first = row[2], block64 = row[3], assign64 = row[4], bps64 = row[5],
                hdr = row[6], file = row[7];
  // the tables are checked before anything is read or stored through them (uniform over the wave)
  bool ok = file >= 0 && file < n_files && start >= 0 && end > start && end <= data_bytes - 8 &&
            end - start <= (INT64_C(1) << 27) && hdr >= 6 && hdr <= 16 && hdr < end - start && block64 >= 1 &&
            block64 <= 65535 && assign64 >= 0 && assign64 <= 10 && bps64 >= 4 && bps64 <= 24 && first >= 0;
  int64_t out_off = 0, stride = 0, total = 0, mono_off = -1;
  int nch = 0;
  if (ok) {
    const int64_t* fl = files + 8 * file;
    out_off = fl[0];
    stride = fl[1];
    nch = (int)(fl[2] >= 1 && fl[2] <= FL_MAXCH ? fl[2] : 0);
    total = fl[4];
    mono_off = fl[5];
    ok = nch > 0 && fl[3] == bps64 && total >= 0 && total <= (INT64_C(1) << 40) && first <= total - block64 &&
         stride >= total && stride <= pcm_len && out_off >= 0 && out_off <= pcm_len - (int64_t)nch * stride &&
         (assign64 < 8 ? assign64 + 1 == nch : nch == 2);
    if (ok && mono && mono_off >= 0) ok = nch <= 2 && mono_off <= mono_len - total;
  }
  if (!ok) {
    if (lane == 0) status[fr] = FL_INVALID;
    return;
  }
  const int block = (int)block64, assign = (int)assign64, bps = (int)bps64;
  int* out0 = pcm + out_off + first;  // channel c's slots: out0[c stride + i], i < block

  crc16_fill_table(crc_tab, lane);
  if (lane == 0) {
    Bits b;
    b.words = reinterpret_cast<const uint32_t*>(data);
    b.n_words = data_bytes >> 2;
    b.base_bit = (uint64_t)start * 8;
    b.end_bit = (uint32_t)(end - start) * 8;
    b.pos = (uint32_t)hdr * 8;
    b.err = 0;
    s_foot = parse_frame(b, sub, out0, stride, nch, block, bps, assign);
    s_err = b.err;
  }
  __syncthreads();
  int err = s_err;
  if (err) {
    if (lane == 0) status[fr] = err;
    return;
  }
  const uint32_t foot = s_foot;  // foot + 2 <= end - start
  const uint8_t* fbytes = data + start;
  const uint32_t crc = wave_crc16([fbytes](int64_t g) { return (uint32_t)fbytes[g]; }, foot, crc_tab, lane);
  if (lane == 0) {
    const uint32_t stored = ((uint32_t)data[start + foot] << 8) | data[start + foot + 1];
    status[fr] = crc == stored ? FL_OK : FL_CRC;
  }

  // C: CONSTANT and VERBATIM subframes
  int max_order = 0;
  for (int c = 0; c < nch; ++c) {
    const Sub& s = sub[c];
    int* out = out0 + c * stride;
    if (s.type == T_CONST) {
      for (int i = lane; i < block; i += 64) out[i] = s.value;
    } else if (s.type == T_VERBATIM) {
      Bits b;
      b.words = reinterpret_cast<const uint32_t*>(data);
      b.n_words = data_bytes >> 2;
      b.base_bit = (uint64_t)start * 8;
      const int sh = 32 - s.bps;
      for (int i = lane; i < block; i += 64)  // inside the frame: parse_frame measured the run
        out[i] = (int)b.peek((uint32_t)s.value + (uint32_t)i * (uint32_t)s.bps) >> sh;
    } else if (s.order > max_order) {
      max_order = s.order;
    }
  }
  // D: predicted subframes
  if (max_order > 16) restore<32>(sub, tile, out0, stride, nch, block, lane);
  else if (max_order > 8) restore<16>(sub, tile, out0, stride, nch, block, lane);
  else if (max_order > 4) restore<8>(sub, tile, out0, stride, nch, block, lane);
  else if (max_order > 0) restore<4>(sub, tile, out0, stride, nch, block, lane);
  __syncthreads();
  // E: wasted bits, stereo decorrelation, outputs
  const float scale = 1.0f / (float)(1 << (bps - 1));
  float* f0 = f32 ? f32 + out_off + first : nullptr;
  float* m0 = (mono && mono_off >= 0) ? mono + mono_off + first : nullptr;
  for (int i = lane; i < block; i += 64) {
    int v[FL_MAXCH];
#pragma unroll
    for (int c = 0; c < FL_MAXCH; ++c)
      v[c] = c < nch ? (int)((uint32_t)out0[c * stride + i] << sub[c].wasted) : 0;
    if (assign == 8) {
      v[1] = v[0] - v[1];
    } else if (assign == 9) {
      v[0] = v[0] + v[1];
    } else if (assign == 10) {
      const int side = v[1], mid = (int)((uint32_t)v[0] << 1) | (side & 1);
      v[0] = (mid + side) >> 1;
      v[1] = (mid - side) >> 1;
    }
#pragma unroll
    for (int c = 0; c < FL_MAXCH; ++c) {
      if (c < nch) {
        out0[c * stride + i] = v[c];
        if (f0) f0[c * stride + i] = (float)v[c] * scale;
      }
    }
    if (m0) {
      const float a = (float)v[0] * scale;
      m0[i] = nch == 1 ? a : __fmul_rn(__fadd_rn(a, (float)v[1] * scale), 0.5f);
    }
  }
}

}  // namespace

int launch_flac_decode(const uint8_t* data, int64_t data_bytes, const int64_t* frames, int64_t n_frames,
                       const int64_t* files, int n_files, int* pcm, float* f32, int64_t pcm_len, float* mono,
                       int64_t mono_len, int* status, hipStream_t st) {
  if (n_frames == 0) return 0;
  if (n_frames < 0 || n_frames > 0x7fffffff || n_files <= 0 || data_bytes < 16 || pcm_len < 0 || mono_len < 0) {
    set_error("flac_decode: need 0 .. 2^31-1 frames, at least one file and a padded byte buffer");
    return -2;
  }
  if (!data || !frames || !files || !pcm || !status) {
    set_error("flac_decode: null argument");
    return -2;
  }
  if ((reinterpret_cast<uintptr_t>(data) & 3) || (data_bytes & 3)) {
    set_error("flac_decode: the byte buffer must be 4-byte aligned and a multiple of 4 bytes long");
    return -2;
  }
  hipLaunchKernelGGL(flac_frame_kernel, dim3((unsigned)n_frames), dim3(64), 0, st, data, data_bytes, frames, n_frames,
                     files, n_files, pcm, f32, pcm_len, mono, mono_len, status);
  NC_HIP(hipGetLastError());
  return 0;
}

}  // namespace nc
