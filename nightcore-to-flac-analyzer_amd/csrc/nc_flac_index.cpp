// nc_flac_index.cpp — host-only FLAC container walk (nc_flac_index in include/ncgpu.h): the
// STREAMINFO block and the table of frames that nc_flac_decode (flac.hip) decodes on the device.
// No HIP header: this file also builds with the host compiler alone (tests/flac_index_main.cpp
// links it under the address and undefined-behaviour sanitizers).
//
// Every read goes through Bytes::at / Bytes::has, which know the buffer's length: damaged or
// truncated input ends in a negative status and an nc_last_error text.
#include <stdint.h>
#include <string.h>

#include <string>

#include "../../include/ncgpu.h"

namespace nc {
void set_error(const std::string& msg);  // nc_capi.cpp (the stand-alone test program has its own)
}

namespace {

struct Bytes {
  const uint8_t* p;
  int64_t n;
  bool has(int64_t pos, int64_t count) const { return pos >= 0 && count >= 0 && pos <= n && count <= n - pos; }
  uint8_t at(int64_t pos) const { return p[pos]; }  // callers check has() first
  uint32_t be(int64_t pos, int count) const {       // big-endian, count <= 4
    uint32_t v = 0;
    for (int i = 0; i < count; ++i) v = (v << 8) | p[pos + i];
    return v;
  }
};

uint8_t crc8(const uint8_t* p, int n) {  // poly 0x07, init 0
  uint8_t c = 0;
  for (int i = 0; i < n; ++i) {
    c ^= p[i];
    for (int b = 0; b < 8; ++b) c = (uint8_t)((c & 0x80) ? ((c << 1) ^ 0x07) : (c << 1));
  }
  return c;
}

struct StreamInfo {
  int64_t rate = 0, channels = 0, bps = 0, total = 0, min_block = 0, max_block = 0;
};

struct FrameHeader {
  int variable = 0;      // blocking strategy bit: the number is a sample number
  int64_t number = 0;    // frame or sample number
  int block = 0, assign = 0, bps = 0, hdr_len = 0;
};

// A frame header at `pos`, parsed fully (sync, reserved codes, UTF-8 style number, block size
// and rate tails, CRC-8).  0: not a header here.  -1: a valid header of an unsupported stream
// (32-bit samples).  1: ok.
int parse_header(const Bytes& d, int64_t pos, const StreamInfo& si, FrameHeader* h) {
  if (!d.has(pos, 5)) return 0;
  if (d.at(pos) != 0xFF || (d.at(pos + 1) & 0xFE) != 0xF8) return 0;  // 0xFFF8 / 0xFFF9
  h->variable = d.at(pos + 1) & 1;
  const int bs_code = d.at(pos + 2) >> 4, sr_code = d.at(pos + 2) & 15;
  const int ch_code = d.at(pos + 3) >> 4, ss_code = (d.at(pos + 3) >> 1) & 7;
  if (d.at(pos + 3) & 1) return 0;                 // reserved bit
  if (bs_code == 0 || sr_code == 15 || ch_code > 10 || ss_code == 3) return 0;  // reserved codes
  int64_t q = pos + 4;
  // the number: 0xxxxxxx, or 110xxxxx .. 11111110 followed by 1 .. 6 continuation bytes
  const uint8_t b0 = d.at(q);
  int extra = 0;
  uint64_t num = 0;
  if (b0 < 0x80) {
    num = b0;
  } else if (b0 < 0xC0 || b0 == 0xFF) {
    return 0;
  } else {
    while (extra < 6 && (b0 & (0x40 >> extra))) ++extra;   // leading ones after the first
    num = b0 & (0x3F >> extra);
  }
  ++q;
  if (!d.has(q, extra)) return 0;
  for (int i = 0; i < extra; ++i, ++q) {
    if ((d.at(q) & 0xC0) != 0x80) return 0;
    num = (num << 6) | (d.at(q) & 0x3F);
  }
  if (!h->variable && extra > 5) return 0;         // a frame number has at most 31 bits
  h->number = (int64_t)num;
  int64_t block;
  if (bs_code == 1) block = 192;
  else if (bs_code <= 5) block = 576 << (bs_code - 2);
  else if (bs_code == 6) {
    if (!d.has(q, 1)) return 0;
    block = (int64_t)d.at(q) + 1;
    q += 1;
  } else if (bs_code == 7) {
    if (!d.has(q, 2)) return 0;
    block = (int64_t)d.be(q, 2) + 1;
    q += 2;
  } else block = 256 << (bs_code - 8);
  if (block > 65535) return 0;
  if (sr_code == 12) q += 1;
  else if (sr_code == 13 || sr_code == 14) q += 2;
  if (!d.has(q, 1)) return 0;
  const int len = (int)(q - pos);
  if (crc8(d.p + pos, len) != d.at(q)) return 0;
  static const int kBits[8] = {0, 8, 12, 0, 16, 20, 24, 32};
  const int bps = ss_code == 0 ? (int)si.bps : kBits[ss_code];
  if (bps == 32) return si.bps == 32 ? -1 : 0;
  if (bps != si.bps) return 0;                    // one sample size per stream here
  if ((ch_code < 8 ? ch_code + 1 : 2) != si.channels) return 0;
  h->block = (int)block;
  h->assign = ch_code;
  h->bps = bps;
  h->hdr_len = len + 1;
  return 1;
}

int fail(int rc, const std::string& msg) {
  nc::set_error("nc_flac_index: " + msg);
  return rc;
}

}  // namespace

extern "C" int nc_flac_index(const uint8_t* data, int64_t n_bytes, int64_t* info, uint8_t* md5, int64_t* frames,
                             int64_t cap, int64_t* n_frames) {
  if (!data || n_bytes < 0 || !info || !n_frames || cap < 0 || (cap > 0 && !frames))
    return fail(-1, "null argument or negative size");
  *n_frames = 0;
  const Bytes d{data, n_bytes};
  int64_t pos = 0;
  if (d.has(0, 10) && d.at(0) == 'I' && d.at(1) == 'D' && d.at(2) == '3') {  // ID3v2: sync-safe size
    const int64_t size = ((int64_t)(d.at(6) & 0x7F) << 21) | ((int64_t)(d.at(7) & 0x7F) << 14) |
                         ((int64_t)(d.at(8) & 0x7F) << 7) | (int64_t)(d.at(9) & 0x7F);
    pos = 10 + size + ((d.at(5) & 0x10) ? 10 : 0);  // flag bit 4: a 10-byte footer follows
    if (!d.has(pos, 0)) return fail(-4, "ID3v2 tag runs past the end of the data");
  }
  if (!d.has(pos, 4)) return fail(-4, "shorter than a stream marker");
  if (d.at(pos) == 'O' && d.at(pos + 1) == 'g' && d.at(pos + 2) == 'g' && d.at(pos + 3) == 'S')
    return fail(-2, "Ogg container (Ogg FLAC) is not supported; only native FLAC streams are");
  if (!(d.at(pos) == 'f' && d.at(pos + 1) == 'L' && d.at(pos + 2) == 'a' && d.at(pos + 3) == 'C'))
    return fail(-2, "no fLaC stream marker");
  pos += 4;
  StreamInfo si;
  bool have_si = false, last = false;
  while (!last) {
    if (!d.has(pos, 4)) return fail(-4, "metadata block header runs past the end of the data");
    last = (d.at(pos) & 0x80) != 0;
    const int type = d.at(pos) & 0x7F;
    const int64_t len = d.be(pos + 1, 3);
    pos += 4;
    if (!d.has(pos, len)) return fail(-4, "metadata block runs past the end of the data");
    if (!have_si) {                                 // STREAMINFO is the first block, always
      if (type != 0 || len < 34) return fail(-4, "the first metadata block is not STREAMINFO");
      si.min_block = d.be(pos, 2);
      si.max_block = d.be(pos + 2, 2);
      const uint64_t packed = ((uint64_t)d.be(pos + 10, 4) << 32) | d.be(pos + 14, 4);
      si.rate = (int64_t)(packed >> 44);
      si.channels = (int64_t)((packed >> 41) & 7) + 1;
      si.bps = (int64_t)((packed >> 36) & 31) + 1;
      si.total = (int64_t)(packed & ((UINT64_C(1) << 36) - 1));
      if (md5)
        for (int i = 0; i < 16; ++i) md5[i] = d.at(pos + 18 + i);
      have_si = true;
    } else if (type == 127) {
      return fail(-4, "invalid metadata block type 127");
    }
    pos += len;
  }
  if (si.bps == 32) return fail(-2, "32-bit samples are not supported");
  if (si.bps < 4 || si.bps > 24) return fail(-2, "bits per sample outside 4 .. 24");
  if (si.rate <= 0) return fail(-4, "STREAMINFO sample rate 0");
  info[0] = si.rate;
  info[1] = si.channels;
  info[2] = si.bps;
  info[3] = si.total;
  info[4] = si.min_block;
  info[5] = si.max_block;
  info[6] = pos;                                   // first byte after the metadata
  info[7] = 0;

  // frames: a candidate header counts only if its number continues the chain (frame number =
  // previous + 1, or sample number = previous + previous block size; the first is 0), which
  // skips byte patterns inside a frame's payload that happen to spell a header
  int64_t count = 0, next_sample = 0, next_frame = 0;
  int variable = -1;
  int64_t* prev_row = nullptr;
  for (int64_t q = pos; q + 1 < n_bytes; ++q) {
    const void* ff = memchr(data + q, 0xFF, (size_t)(n_bytes - 1 - q));  // the next possible sync byte
    if (!ff) break;
    q = static_cast<const uint8_t*>(ff) - data;
    if ((d.at(q + 1) & 0xFE) != 0xF8) continue;
    FrameHeader h;
    const int r = parse_header(d, q, si, &h);
    if (r < 0) return fail(-2, "32-bit samples are not supported");
    if (r == 0) continue;
    if (variable >= 0 && h.variable != variable) continue;
    if (h.number != (h.variable ? next_sample : next_frame)) continue;
    variable = h.variable;
    if (count < cap) {
      int64_t* row = frames + 8 * count;
      row[0] = q;
      row[1] = n_bytes;
      row[2] = next_sample;
      row[3] = h.block;
      row[4] = h.assign;
      row[5] = h.bps;
      row[6] = h.hdr_len;
      row[7] = 0;                                  // file index: the caller's, in a batched decode
      if (prev_row) prev_row[1] = q;
      prev_row = row;
    }
    ++count;
    next_sample += h.block;
    next_frame += 1;
    q += h.hdr_len - 1;                            // a frame is longer than its header
  }
  *n_frames = count;
  if (si.total == 0) info[3] = next_sample;
  else if (next_sample != si.total)
    return fail(-4, "the frames hold " + std::to_string(next_sample) + " samples per channel, STREAMINFO says " +
                        std::to_string(si.total) + " (truncated or damaged stream)");
  if (cap > 0 && count > cap) return fail(-3, "frame table capacity too small");
  return 0;
}
