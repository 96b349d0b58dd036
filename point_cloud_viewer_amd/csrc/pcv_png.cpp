// pcv_png.cpp — host-only PNG reader for xray quadtree tiles (pcv_png_decode): what the reference reads back with the
// image crate when it merges partial quadtrees (xray/src/generation.rs:726-759 build_node -> image::open), and the host
// PNG writers (pcv_xray_png_encode_ex: stored blocks, or the run-length deflate stream of pcv_xray_png_dev.h). No HIP, no
// context, no zlib: the file compiles with a plain C++ compiler, which is how the sanitizer drivers of the tests build it.
//
//   container   signature, chunk walk with every CRC checked, IHDR first, IDAT bodies concatenated, IEND required;
//               ancillary chunks (lower-case first letter) and PLTE are skipped
//   zlib        CMF / FLG check, no preset dictionary, inflate (stored, fixed and dynamic Huffman blocks), Adler-32
//   inflate     canonical Huffman decoding one bit at a time over count / symbol tables (RFC 1951 3.2.2); the output is
//               bounded by the h * (1 + 4 w) bytes the header promises, a distance may not reach before its start
//   rows        filters None, Sub, Up, Average, Paeth undone in place, 4 bytes per pixel (RFC 2083 6)
//
// Inflate is sequential and dominates; Average and Paeth are serial along both axes; a tile is 256 KiB. That is why the
// whole reader stays on the host.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/pcv_hip.h"
#include "pcv_xray_png_dev.h"

namespace {

thread_local std::string g_host_error;

constexpr uint32_t kMaxPngEdge = 32768;  // the largest tile pcv_xray_run makes

struct Crc32Table {
  uint32_t t[256];
  Crc32Table() {
    for (uint32_t i = 0; i < 256; ++i) {
      uint32_t c = i;
      for (int k = 0; k < 8; ++k) c = c & 1 ? 0xedb88320u ^ (c >> 1) : c >> 1;
      t[i] = c;
    }
  }
};
uint32_t crc32_of(const uint8_t* p, uint64_t n) {
  static const Crc32Table table;
  uint32_t crc = 0xffffffffu;
  for (uint64_t i = 0; i < n; ++i) crc = table.t[(crc ^ p[i]) & 255u] ^ (crc >> 8);
  return crc ^ 0xffffffffu;
}

uint32_t be32(const uint8_t* p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | (uint32_t)p[3]; }

// LSB-first bit reader over [p, p + n): a byte is fetched only when a bit of it is needed, so after a block fewer than 8
// bits are pending and `pos` is the next whole byte
struct BitReader {
  const uint8_t* p;
  uint64_t n, pos = 0;
  uint32_t buf = 0;
  int cnt = 0;
  bool bad = false;  // ran past the end
  uint32_t bits(int need) {  // need <= 16
    while (cnt < need) {
      if (pos >= n) {
        bad = true;
        return 0;
      }
      buf |= (uint32_t)p[pos++] << cnt;
      cnt += 8;
    }
    const uint32_t v = buf & ((1u << need) - 1u);
    buf >>= need;
    cnt -= need;
    return v;
  }
};

constexpr int kMaxBits = 15, kMaxLitLen = 288, kMaxDist = 30;
struct Huffman {
  uint16_t count[kMaxBits + 1];
  uint16_t symbol[kMaxLitLen];
};

// code lengths -> canonical tables. 0: complete; > 0: incomplete (codes left over); < 0: over-subscribed
int huffman_build(Huffman& h, const uint8_t* length, int n) {
  for (int l = 0; l <= kMaxBits; ++l) h.count[l] = 0;
  for (int s = 0; s < n; ++s) ++h.count[length[s]];
  if (h.count[0] == n) return 0;  // no codes: complete, and every decode fails
  int left = 1;
  for (int l = 1; l <= kMaxBits; ++l) {
    left <<= 1;
    left -= h.count[l];
    if (left < 0) return left;
  }
  uint16_t offs[kMaxBits + 1];
  offs[1] = 0;
  for (int l = 1; l < kMaxBits; ++l) offs[l + 1] = (uint16_t)(offs[l] + h.count[l]);
  for (int s = 0; s < n; ++s)
    if (length[s]) h.symbol[offs[length[s]]++] = (uint16_t)s;
  return left;
}

// -1: a code no symbol has, or the input ended
int huffman_decode(BitReader& br, const Huffman& h) {
  int code = 0, first = 0, index = 0;
  for (int l = 1; l <= kMaxBits; ++l) {
    code |= (int)br.bits(1);
    if (br.bad) return -1;
    const int count = h.count[l];
    if (code - count < first) return h.symbol[index + (code - first)];
    index += count;
    first += count;
    first <<= 1;
    code <<= 1;
  }
  return -1;
}

const uint16_t kLenBase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
const uint8_t kLenExtra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
const uint16_t kDistBase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
const uint8_t kDistExtra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};

struct Sink {  // the h * (1 + 4 w) bytes the header promises
  uint8_t* out;
  uint64_t cap, len = 0;
};

// one Huffman-coded block. nullptr: fine; otherwise what is wrong with the stream
const char* inflate_codes(BitReader& br, Sink& o, const Huffman& lit, const Huffman& dist) {
  for (;;) {
    int sym = huffman_decode(br, lit);
    if (sym < 0) return br.bad ? "deflate stream ends inside a block" : "invalid literal / length code";
    if (sym < 256) {
      if (o.len >= o.cap) return "more image data than the header promises";
      o.out[o.len++] = (uint8_t)sym;
    } else if (sym == 256) {
      return nullptr;
    } else {
      sym -= 257;
      if (sym >= 29) return "invalid length symbol";
      const uint32_t len = kLenBase[sym] + br.bits(kLenExtra[sym]);
      const int ds = huffman_decode(br, dist);
      if (ds < 0) return br.bad ? "deflate stream ends inside a block" : "invalid distance code";
      if (ds >= kMaxDist) return "invalid distance symbol";
      const uint64_t d = kDistBase[ds] + br.bits(kDistExtra[ds]);
      if (br.bad) return "deflate stream ends inside a block";
      if (d > o.len) return "distance reaches before the start of the output";
      if (len > o.cap - o.len) return "more image data than the header promises";
      for (uint32_t k = 0; k < len; ++k, ++o.len) o.out[o.len] = o.out[o.len - d];  // may overlap: byte by byte
    }
  }
}

const char* inflate_stored(BitReader& br, Sink& o) {
  br.buf = 0;  // to the next byte boundary
  br.cnt = 0;
  if (br.n - br.pos < 4) return "deflate stream ends inside a stored block header";
  const uint32_t len = br.p[br.pos] | (uint32_t)br.p[br.pos + 1] << 8, nlen = br.p[br.pos + 2] | (uint32_t)br.p[br.pos + 3] << 8;
  br.pos += 4;
  if ((len ^ 0xffffu) != nlen) return "stored block length and its complement disagree";
  if (br.n - br.pos < len) return "deflate stream ends inside a stored block";
  if (len > o.cap - o.len) return "more image data than the header promises";
  std::memcpy(o.out + o.len, br.p + br.pos, len);
  o.len += len;
  br.pos += len;
  return nullptr;
}

const char* inflate_fixed(BitReader& br, Sink& o) {
  uint8_t length[kMaxLitLen];
  int s = 0;
  for (; s < 144; ++s) length[s] = 8;
  for (; s < 256; ++s) length[s] = 9;
  for (; s < 280; ++s) length[s] = 7;
  for (; s < kMaxLitLen; ++s) length[s] = 8;
  Huffman lit, dist;
  huffman_build(lit, length, kMaxLitLen);
  for (s = 0; s < kMaxDist; ++s) length[s] = 5;
  huffman_build(dist, length, kMaxDist);
  return inflate_codes(br, o, lit, dist);
}

const char* inflate_dynamic(BitReader& br, Sink& o) {
  static const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  const int nlen = (int)br.bits(5) + 257, ndist = (int)br.bits(5) + 1, ncode = (int)br.bits(4) + 4;
  if (br.bad) return "deflate stream ends inside a block header";
  if (nlen > 286 || ndist > kMaxDist) return "too many length or distance codes";
  uint8_t length[kMaxLitLen + kMaxDist + 16] = {};
  for (int i = 0; i < ncode; ++i) length[order[i]] = (uint8_t)br.bits(3);
  if (br.bad) return "deflate stream ends inside a block header";
  Huffman lencode;
  if (huffman_build(lencode, length, 19) != 0) return "code length code is not complete";
  uint8_t lens[kMaxLitLen + kMaxDist] = {};
  int i = 0;
  while (i < nlen + ndist) {
    const int sym = huffman_decode(br, lencode);
    if (sym < 0) return br.bad ? "deflate stream ends inside a block header" : "invalid code length code";
    if (sym < 16) {
      lens[i++] = (uint8_t)sym;
      continue;
    }
    uint8_t prev = 0;
    int rep;
    if (sym == 16) {
      if (i == 0) return "code length repeat without a previous length";
      prev = lens[i - 1];
      rep = 3 + (int)br.bits(2);
    } else if (sym == 17) {
      rep = 3 + (int)br.bits(3);
    } else {
      rep = 11 + (int)br.bits(7);
    }
    if (br.bad) return "deflate stream ends inside a block header";
    if (i + rep > nlen + ndist) return "code length repeat past the end";
    while (rep--) lens[i++] = prev;
  }
  if (lens[256] == 0) return "no end-of-block code";
  Huffman lit, dist;
  int err = huffman_build(lit, lens, nlen);
  // an incomplete code is accepted only as zlib accepts it: every used code of length 1
  if (err < 0 || (err > 0 && nlen - lit.count[0] != lit.count[1])) return "invalid literal / length code lengths";
  err = huffman_build(dist, lens + nlen, ndist);
  if (err < 0 || (err > 0 && ndist - dist.count[0] != dist.count[1])) return "invalid distance code lengths";
  return inflate_codes(br, o, lit, dist);
}

uint32_t adler32_of(const uint8_t* p, uint64_t n) {
  uint32_t s1 = 1, s2 = 0;
  for (uint64_t i = 0; i < n;) {  // reduced at most every 5 552 bytes
    const uint64_t m = n - i < 5552 ? n - i : 5552;
    for (uint64_t j = 0; j < m; ++j) {
      s1 += p[i + j];
      s2 += s1;
    }
    s1 %= 65521u;
    s2 %= 65521u;
    i += m;
  }
  return s2 << 16 | s1;
}

// the zlib stream z[0, n) into exactly `cap` bytes
const char* zlib_inflate(const uint8_t* z, uint64_t n, uint8_t* out, uint64_t cap) {
  if (n < 2) return "zlib stream shorter than its header";
  if ((z[0] & 0x0f) != 8 || (z[0] >> 4) > 7 || (((uint32_t)z[0] << 8) | z[1]) % 31 != 0) return "bad zlib header";
  if (z[1] & 0x20) return "zlib stream asks for a preset dictionary";
  BitReader br{z + 2, n - 2};
  Sink o{out, cap};
  for (;;) {
    const uint32_t last = br.bits(1), type = br.bits(2);
    if (br.bad) return "deflate stream ends before its last block";
    const char* e = type == 0 ? inflate_stored(br, o) : type == 1 ? inflate_fixed(br, o) : type == 2 ? inflate_dynamic(br, o) : "reserved block type";
    if (e) return e;
    if (last) break;
  }
  if (o.len != cap) return "less image data than the header promises";
  if (br.n - br.pos < 4) return "zlib stream ends before its Adler-32";
  if (be32(br.p + br.pos) != adler32_of(out, cap)) return "Adler-32 mismatch";
  return nullptr;
}

int paeth(int a, int b, int c) {
  const int p = a + b - c, pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
  return pa <= pb && pa <= pc ? a : (pb <= pc ? b : c);
}

// rows of 1 + 4 w bytes (filter byte first), unfiltered in place. false: a filter byte above 4
bool unfilter(uint8_t* raw, uint32_t w, uint32_t h) {
  const uint64_t stride = 1 + 4ull * w, n = 4ull * w;
  for (uint32_t y = 0; y < h; ++y) {
    uint8_t* cur = raw + y * stride + 1;
    const uint8_t* up = y ? cur - stride : nullptr;
    switch (cur[-1]) {
      case 0:
        break;
      case 1:
        for (uint64_t i = 4; i < n; ++i) cur[i] = (uint8_t)(cur[i] + cur[i - 4]);
        break;
      case 2:
        if (up)
          for (uint64_t i = 0; i < n; ++i) cur[i] = (uint8_t)(cur[i] + up[i]);
        break;
      case 3:
        for (uint64_t i = 0; i < n; ++i) cur[i] = (uint8_t)(cur[i] + (((i >= 4 ? cur[i - 4] : 0) + (up ? up[i] : 0)) >> 1));
        break;
      case 4:
        for (uint64_t i = 0; i < n; ++i)
          cur[i] = (uint8_t)(cur[i] + paeth(i >= 4 ? cur[i - 4] : 0, up ? up[i] : 0, (up && i >= 4) ? up[i - 4] : 0));
        break;
      default:
        return false;
    }
  }
  return true;
}

}  // namespace

int pcv_host_fail(int code, const std::string& msg) {
  g_host_error = msg;
  return code;
}

extern "C" const char* pcv_host_last_error(void) { return g_host_error.c_str(); }

extern "C" int pcv_png_decode(const uint8_t* file, uint64_t len, uint32_t* w, uint32_t* h, uint8_t* rgba, uint64_t capacity) {
  static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
  if (!file) return pcv_host_fail(PCV_E_INVALID, "png: null input");
  if (len < 8 || std::memcmp(file, sig, 8) != 0) return pcv_host_fail(PCV_E_IO, "png: no PNG signature");
  uint64_t pos = 8;
  uint32_t W = 0, H = 0;
  bool have_ihdr = false, have_iend = false;
  std::vector<uint8_t> z;
  while (!have_iend) {
    if (len - pos < 12) return pcv_host_fail(PCV_E_IO, "png: file ends inside a chunk");
    const uint32_t n = be32(file + pos);
    const uint8_t* type = file + pos + 4;
    if (n > len - pos - 12) return pcv_host_fail(PCV_E_IO, "png: file ends inside a chunk");
    if (crc32_of(type, 4ull + n) != be32(type + 4 + n)) return pcv_host_fail(PCV_E_IO, "png: chunk CRC mismatch");
    const uint8_t* body = type + 4;
    if (!have_ihdr) {
      if (std::memcmp(type, "IHDR", 4) != 0 || n != 13) return pcv_host_fail(PCV_E_IO, "png: the first chunk is not a 13-byte IHDR");
      W = be32(body);
      H = be32(body + 4);
      if (W == 0 || H == 0) return pcv_host_fail(PCV_E_IO, "png: zero width or height");
      if (body[8] != 8 || body[9] != 6)
        return pcv_host_fail(PCV_E_INVALID, "png: colour type " + std::to_string(body[9]) + " at depth " + std::to_string(body[8]) +
                                                " (only RGBA8, colour type 6 at depth 8, is read)");
      if (body[10] != 0 || body[11] != 0) return pcv_host_fail(PCV_E_INVALID, "png: unknown compression or filter method");
      if (body[12] != 0) return pcv_host_fail(PCV_E_INVALID, "png: interlaced images are not read");
      if (W > kMaxPngEdge || H > kMaxPngEdge) return pcv_host_fail(PCV_E_INVALID, "png: wider or taller than 32768 pixels");
      have_ihdr = true;
    } else if (std::memcmp(type, "IDAT", 4) == 0) {
      z.insert(z.end(), body, body + n);
    } else if (std::memcmp(type, "IEND", 4) == 0) {
      have_iend = true;
    } else if (std::memcmp(type, "IHDR", 4) == 0) {
      return pcv_host_fail(PCV_E_IO, "png: a second IHDR");
    } else if (!(type[0] & 0x20) && std::memcmp(type, "PLTE", 4) != 0) {
      return pcv_host_fail(PCV_E_INVALID, "png: unknown critical chunk");
    }
    pos += 12ull + n;
  }
  if (w) *w = W;
  if (h) *h = H;
  if (!rgba) return PCV_OK;  // the size alone
  const uint64_t need = 4ull * W * H, raw_len = (uint64_t)H * (1 + 4ull * W);
  if (capacity < need) return pcv_host_fail(PCV_E_INVALID, "png: capacity below 4 x width x height bytes");
  // deflate expands at most 1032 : 1 (a 258-byte match per 2 bits): a shorter stream cannot hold the image
  if (raw_len / 1032 > z.size()) return pcv_host_fail(PCV_E_IO, "png: less image data than the header promises");
  uint8_t* raw = new (std::nothrow) uint8_t[raw_len];
  if (!raw) return pcv_host_fail(PCV_E_OOM, "png: no host memory for the scanlines");
  const char* e = zlib_inflate(z.data(), z.size(), raw, raw_len);
  if (!e && !unfilter(raw, W, H)) e = "unknown row filter";
  if (e) {
    delete[] raw;
    return pcv_host_fail(PCV_E_IO, std::string("png: ") + e);
  }
  for (uint32_t y = 0; y < H; ++y) std::memcpy(rgba + (uint64_t)y * 4 * W, raw + (uint64_t)y * (1 + 4ull * W) + 1, 4ull * W);
  delete[] raw;
  return PCV_OK;
}

// ---- writers: RGBA8, colour type 6, depth 8, one IDAT --------------------------------------------------------------------
namespace {

uint32_t crc32_table[256];
std::once_flag crc32_once;

constexpr uint64_t kStored = 65535;  // bytes per stored deflate block

void put_be32(uint8_t* o, uint32_t v) {
  o[0] = (uint8_t)(v >> 24);
  o[1] = (uint8_t)(v >> 16);
  o[2] = (uint8_t)(v >> 8);
  o[3] = (uint8_t)v;
}

// signature and IHDR: 33 bytes
uint8_t* put_head(uint8_t* o, uint32_t w, uint32_t h) {
  static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
  std::memcpy(o, sig, 8);
  o += 8;
  put_be32(o, 13);
  uint8_t* t = o + 4;
  std::memcpy(t, "IHDR", 4);
  put_be32(t + 4, w);
  put_be32(t + 8, h);
  t[12] = 8;  // bit depth
  t[13] = 6;  // RGBA
  t[14] = 0;  // deflate
  t[15] = 0;  // adaptive filtering (a filter byte per row)
  t[16] = 0;  // no interlace
  put_be32(t + 17, pcv_crc32_update(0xffffffffu, t, 17) ^ 0xffffffffu);
  return t + 21;
}

uint8_t* put_iend(uint8_t* o) {
  put_be32(o, 0);
  std::memcpy(o + 4, "IEND", 4);
  put_be32(o + 8, pcv_crc32_update(0xffffffffu, o + 4, 4) ^ 0xffffffffu);
  return o + 12;
}

// LSB-first bit writer into a buffer sized by the caller from pcv_png_band_bound
struct BitWriter {
  uint8_t* o;
  uint64_t acc = 0;
  uint32_t cnt = 0;
  void put(uint32_t bits, uint32_t nbits) {
    acc |= (uint64_t)bits << cnt;
    cnt += nbits;
    while (cnt >= 8) {
      *o++ = (uint8_t)acc;
      acc >>= 8;
      cnt -= 8;
    }
  }
  void pad() {
    if (cnt) {
      *o++ = (uint8_t)acc;
      acc = 0;
      cnt = 0;
    }
  }
};

// the zlib stream of pcv_xray_png_dev.h into z (pcv_png_stream_bound(w, h) bytes); returns its length
uint64_t deflate_stream(const uint8_t* rgba, uint32_t w, uint32_t h, uint8_t* z) {
  const uint64_t row = 1 + 4ull * w;
  const uint32_t per_band = PCV_XRAY_PNG_BAND_ROWS(w);
  std::vector<uint8_t> band(per_band * row);
  BitWriter bw{z};
  bw.put(0x78, 8);
  bw.put(0x01, 8);
  uint32_t s1 = 1, s2 = 0;
  for (uint32_t y0 = 0; y0 < h; y0 += per_band) {
    const uint32_t rows = std::min(per_band, h - y0);
    const uint64_t n = rows * row;
    for (uint64_t j = 0; j < n; ++j) band[j] = (uint8_t)pcv_png_filtered(rgba, w, y0 + (uint32_t)(j / row), (uint32_t)(j % row));
    for (uint64_t i = 0; i < n;) {  // Adler-32, reduced at most every 5 552 bytes
      const uint64_t m = std::min<uint64_t>(5552, n - i);
      for (uint64_t j = 0; j < m; ++j) {
        s1 += band[i + j];
        s2 += s1;
      }
      s1 %= 65521u;
      s2 %= 65521u;
      i += m;
    }
    bw.put(2, 3);  // BFINAL 0, BTYPE 01
    for (uint64_t j = 0; j < n;) {
      uint64_t e = j + 1;
      while (e < n && band[e] == band[j]) ++e;
      pcv_png_run_emit((uint32_t)(e - j), band[j], [&](uint32_t bits, uint32_t nbits) { bw.put(bits, nbits); });
      j = e;
    }
    bw.put(0, 7);                                 // end of block
    bw.put(y0 + rows == h ? 1u : 0u, 3);          // the empty stored block
    bw.pad();
    bw.put(0x0000, 16);
    bw.put(0xffff, 16);
  }
  bw.put(s2 >> 8, 8);
  bw.put(s2 & 255u, 8);
  bw.put(s1 >> 8, 8);
  bw.put(s1 & 255u, 8);
  return (uint64_t)(bw.o - z);
}

}  // namespace

uint32_t pcv_crc32_update(uint32_t crc, const uint8_t* p, uint64_t n) {
  std::call_once(crc32_once, [] {
    for (uint32_t i = 0; i < 256; ++i) {
      uint32_t c = i;
      for (int k = 0; k < 8; ++k) c = c & 1 ? 0xedb88320u ^ (c >> 1) : c >> 1;
      crc32_table[i] = c;
    }
  });
  for (uint64_t i = 0; i < n; ++i) crc = crc32_table[(crc ^ p[i]) & 255u] ^ (crc >> 8);
  return crc;
}

uint64_t pcv_png_stored_size(uint32_t w, uint32_t h) {
  const uint64_t raw = (uint64_t)h * (1 + 4ull * w);
  const uint64_t blocks = (raw + kStored - 1) / kStored;
  return kPcvPngWrap + 2 + 5 * blocks + raw + 4;
}

// filter byte 0 on every row, zlib with stored deflate blocks
void pcv_png_stored_encode(const uint8_t* rgba, uint32_t w, uint32_t h, uint8_t* out) {
  uint8_t* o = put_head(out, w, h);
  // IDAT: zlib header (deflate, 32 K window, no dictionary, FCHECK), stored blocks, Adler-32
  uint8_t* t = o + 4;
  std::memcpy(t, "IDAT", 4);
  o = t + 4;
  *o++ = 0x78;
  *o++ = 0x01;
  const uint64_t row = 1 + 4ull * w, raw = (uint64_t)h * row;
  uint32_t s1 = 1, s2 = 0;
  uint64_t done = 0;
  uint8_t* blk = nullptr;
  uint64_t room = 0;
  auto put = [&](const uint8_t* p, uint64_t n) {  // appends scanline bytes, opening stored blocks as they fill
    while (n) {
      if (room == 0) {
        const uint64_t len = std::min<uint64_t>(kStored, raw - done);
        blk = o;
        blk[0] = done + len == raw ? 1 : 0;  // BFINAL, BTYPE = 00
        blk[1] = (uint8_t)len;
        blk[2] = (uint8_t)(len >> 8);
        blk[3] = (uint8_t)~len;
        blk[4] = (uint8_t)(~len >> 8);
        o += 5;
        room = len;
      }
      const uint64_t k = std::min(n, room);
      std::memcpy(o, p, k);
      for (uint64_t i = 0; i < k;) {  // Adler-32, reduced at most every 5 552 bytes
        const uint64_t m = std::min<uint64_t>(5552, k - i);
        for (uint64_t j = 0; j < m; ++j) {
          s1 += p[i + j];
          s2 += s1;
        }
        s1 %= 65521u;
        s2 %= 65521u;
        i += m;
      }
      o += k;
      p += k;
      n -= k;
      room -= k;
      done += k;
    }
  };
  const uint8_t filter = 0;
  for (uint32_t y = 0; y < h; ++y) {
    put(&filter, 1);
    put(rgba + (uint64_t)y * 4 * w, 4ull * w);
  }
  put_be32(o, s2 << 16 | s1);
  o += 4;
  put_be32(t - 4, (uint32_t)(o - t - 4));
  put_be32(o, pcv_crc32_update(0xffffffffu, t, (uint64_t)(o - t)) ^ 0xffffffffu);
  put_iend(o + 4);
}

void pcv_png_wrap(uint32_t w, uint32_t h, const uint8_t* z, uint64_t zlen, uint8_t* out) {
  uint8_t* o = put_head(out, w, h);
  put_be32(o, (uint32_t)zlen);
  std::memcpy(o + 4, "IDAT", 4);
  if (o + 8 != z) std::memmove(o + 8, z, zlen);  // the stream may have been made in place
  put_be32(o + 8 + zlen, pcv_crc32_update(0xffffffffu, o + 4, 4 + zlen) ^ 0xffffffffu);
  put_iend(o + 12 + zlen);
}

extern "C" uint64_t pcv_xray_png_bound(uint32_t w, uint32_t h, int mode) {
  if (w == 0 || h == 0 || w > (1u << 30) / 4) return 0;
  if (mode == PCV_XRAY_PNG_STORED) return pcv_png_stored_size(w, h);
  if (mode != PCV_XRAY_PNG_DEFLATE || w > PCV_XRAY_PNG_DEFLATE_MAX_EDGE || h > PCV_XRAY_PNG_DEFLATE_MAX_EDGE) return 0;
  return kPcvPngWrap + pcv_png_stream_bound(w, h);
}

extern "C" int pcv_xray_png_encode_ex(const uint8_t* rgba, uint32_t w, uint32_t h, int mode, uint8_t* out, uint64_t capacity,
                                      uint64_t* needed) {
  if (w == 0 || h == 0 || w > (1u << 30) / 4 || (!rgba && out)) return pcv_host_fail(PCV_E_INVALID, "png: bad image arguments");
  if (mode == PCV_XRAY_PNG_STORED) {
    const uint64_t n = pcv_png_stored_size(w, h);
    if (needed) *needed = n;
    if (out && capacity >= n) pcv_png_stored_encode(rgba, w, h, out);
    return PCV_OK;
  }
  if (mode != PCV_XRAY_PNG_DEFLATE) return pcv_host_fail(PCV_E_INVALID, "png: unknown mode");
  if (w > PCV_XRAY_PNG_DEFLATE_MAX_EDGE || h > PCV_XRAY_PNG_DEFLATE_MAX_EDGE)
    return pcv_host_fail(PCV_E_INVALID, "png: deflate mode takes images of at most 8192 x 8192 pixels");
  const uint64_t bound = kPcvPngWrap + pcv_png_stream_bound(w, h);
  if (!rgba) {
    if (needed) *needed = bound;
    return PCV_OK;
  }
  uint8_t* file = new (std::nothrow) uint8_t[bound];
  if (!file) return pcv_host_fail(PCV_E_OOM, "png: no host memory for the stream");
  uint8_t* z = file + 8 + 25 + 8;  // where the IDAT's data goes
  const uint64_t zlen = deflate_stream(rgba, w, h, z);
  const uint64_t n = kPcvPngWrap + zlen;
  if (needed) *needed = n;
  if (out && capacity >= n) {
    pcv_png_wrap(w, h, z, zlen, file);
    std::memcpy(out, file, n);
  }
  delete[] file;
  return PCV_OK;
}

extern "C" int pcv_xray_png_encode(const uint8_t* rgba, uint32_t w, uint32_t h, uint8_t* out, uint64_t capacity, uint64_t* needed) {
  if (w == 0 || h == 0 || w > (1u << 30) / 4 || (!rgba && out)) return PCV_E_INVALID;
  return pcv_xray_png_encode_ex(rgba, w, h, PCV_XRAY_PNG_STORED, out, capacity, needed);
}
