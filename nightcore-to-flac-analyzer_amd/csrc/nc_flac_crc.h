// nc_flac_crc.h — FLAC's CRC-16 (poly 0x8005, init 0) by a whole wave, shared by the decoder
// (flac.hip) and the encoder (flac_enc.hip): 64 equal chunks, joined by
// crc(A || B) = crc(A) x^(8 |B|) + crc(B) in GF(2)[x] / (x^16 + x^15 + x^2 + 1).
#pragma once
#include <stdint.h>

namespace nc {

__device__ inline uint32_t gf_mulmod(uint32_t a, uint32_t m) {  // a m mod x^16 + 0x8005
  uint32_t r = 0;
  for (int i = 15; i >= 0; --i) {
    r = ((r << 1) ^ ((r & 0x8000) ? 0x8005u : 0u)) & 0xffff;
    if ((m >> i) & 1) r ^= a;
  }
  return r;
}

// tab[0 .. 256): the byte-wise table, filled by the 64 lanes (a barrier must follow)
template <class T>
__device__ inline void crc16_fill_table(T* tab, int lane) {
  for (int i = lane; i < 256; i += 64) {
    uint32_t c = (uint32_t)i << 8;
    for (int k = 0; k < 8; ++k) c = ((c << 1) ^ ((c & 0x8000) ? 0x8005u : 0u)) & 0xffff;
    tab[i] = (T)c;
  }
}

// CRC-16 of the bytes byte_at(0 .. n) by the whole wave; the result is valid in lane 0
template <class T, class Fetch>
__device__ inline uint32_t wave_crc16(Fetch byte_at, uint32_t n, const T* tab, int lane) {
  const uint32_t chunk = (n + 63) / 64;
  const int64_t pad = (int64_t)chunk * 64 - n;  // leading zero bytes leave a CRC with init 0 unchanged
  uint32_t crc = 0, xl = 1;                     // xl = x^(8 chunk)
  for (uint32_t j = 0; j < chunk; ++j) {
    const int64_t g = (int64_t)lane * chunk + j - pad;
    const uint32_t byte = g >= 0 ? byte_at(g) : 0;
    crc = ((crc << 8) ^ tab[(crc >> 8) ^ byte]) & 0xffff;
    xl = ((xl << 8) ^ tab[xl >> 8]) & 0xffff;
  }
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t right = __shfl_down(crc, d, 64);
    crc = gf_mulmod(crc, xl) ^ right;
    xl = gf_mulmod(xl, xl);
  }
  return crc;
}

}  // namespace nc
