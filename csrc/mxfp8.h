// MXFP8 wire format of the dense reduce rounds: sizes, the e4m3 codec and
// a host reference of quantize / dequantize. Plain C++, no HIP calls — the
// kernels (mxfp8.hip) share the scale rule and the software codec, the
// tests run the host reference on a machine without a GPU.
//
// A superblock packs 512 fp32 elements into 528 bytes: 16 scale bytes (one
// E8M0 byte, value 2^(byte-127), per block of 32 consecutive elements),
// then 512 OCP e4m3fn codes in element order. n elements take
// ceil(n/512) superblocks; elements past n count as +0.0.
//
// Scale of a block: amax = max|x|, be = exponent field of amax,
// byte = max(be - 8, 0), and one more if amax * 2^(127-byte) > 448 (so
// the block's largest element never saturates). Code of an element:
// e4m3fn_rne(clamp(x * 2^(127-byte), -448, 448)). Inputs are finite with
// |x| either 0 or in [2^-100, 2^100].
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define XPS_MX_HD __host__ __device__
#else
#define XPS_MX_HD
#endif

namespace xps {
namespace mx {

static const size_t kBlockElems = 32;        // elements per scale byte
static const size_t kSuperElems = 512;       // elements per superblock
static const size_t kSuperScales = 16;       // scale bytes heading a superblock
static const size_t kSuperBytes = 528;       // packed bytes per superblock (33 x 16)
static const size_t kSuperF32Bytes = 2048;   // the same elements as fp32
static const float kE4m3Max = 448.0f;

XPS_MX_HD inline size_t MxSuperblocks(size_t n) { return (n + kSuperElems - 1) / kSuperElems; }
XPS_MX_HD inline size_t MxPackedBytes(size_t n) { return MxSuperblocks(n) * kSuperBytes; }

XPS_MX_HD inline uint32_t F32Bits(float f) {
  union {
    float f;
    uint32_t u;
  } c;
  c.f = f;
  return c.u;
}

XPS_MX_HD inline float BitsF32(uint32_t u) {
  union {
    float f;
    uint32_t u;
  } c;
  c.u = u;
  return c.f;
}

// E8M0 byte of a block whose largest magnitude is amax (>= 0)
XPS_MX_HD inline uint32_t ScaleByte(float amax) {
  uint32_t be = (F32Bits(amax) >> 23) & 0xffu;
  uint32_t byte = be > 8 ? be - 8 : 0;
  // 2^(127-byte): exponent field 254 - byte, in [6, 254] for every byte
  if (amax * BitsF32((254u - byte) << 23) > kE4m3Max) ++byte;
  return byte;
}

// 2^(127-byte), the exact multiplier that brings a block into e4m3 range
XPS_MX_HD inline float InvScale(uint32_t byte) { return BitsF32((254u - byte) << 23); }

// Software e4m3fn encode, round to nearest even; |f| <= 448 (clamped by
// the caller). Subnormal codes (below 2^-6) are multiples of 2^-9.
XPS_MX_HD inline uint8_t E4m3Encode(float f) {
  uint32_t bits = F32Bits(f);
  uint32_t sign = (bits >> 24) & 0x80u;
  bits &= 0x7fffffffu;
  if (bits < 0x3c800000u) {  // below 2^-6: x * 2^9 is exact, rint rounds to even
    return static_cast<uint8_t>(sign | static_cast<uint32_t>(rintf(BitsF32(bits) * 512.0f)));
  }
  bits += 0x7ffffu + ((bits >> 20) & 1u);  // RNE to 3 mantissa bits (may carry)
  uint32_t e = (bits >> 23) - 120u;         // e4m3 bias 7 against fp32's 127
  return static_cast<uint8_t>(sign | (e << 3) | ((bits >> 20) & 7u));
}

XPS_MX_HD inline float E4m3Decode(uint8_t c) {
  uint32_t sign = static_cast<uint32_t>(c & 0x80u) << 24;
  uint32_t e = (c >> 3) & 15u, m = c & 7u;
  if (e == 15u && m == 7u) return BitsF32(sign | 0x7fc00000u);  // the format's NaN
  if (e == 0) return BitsF32(sign | F32Bits(static_cast<float>(m) * 0.001953125f));
  return BitsF32(sign | ((e + 120u) << 23) | (m << 20));
}

XPS_MX_HD inline float Clamp448(float x) {
  return x > kE4m3Max ? kE4m3Max : (x < -kE4m3Max ? -kE4m3Max : x);
}

// packed <- Q(src[0, n)); writes MxPackedBytes(n) bytes
inline void MxQuantizeHost(const float* src, size_t n, uint8_t* packed) {
  for (size_t sb = 0; sb < MxSuperblocks(n); ++sb) {
    uint8_t* scales = packed + sb * kSuperBytes;
    uint8_t* codes = scales + kSuperScales;
    for (size_t b = 0; b < kSuperScales; ++b) {
      size_t base = sb * kSuperElems + b * kBlockElems;
      float x[kBlockElems];
      float amax = 0.0f;
      for (size_t i = 0; i < kBlockElems; ++i) {
        x[i] = base + i < n ? src[base + i] : 0.0f;
        float a = std::fabs(x[i]);
        if (a > amax) amax = a;
      }
      uint32_t byte = ScaleByte(amax);
      float inv = InvScale(byte);
      scales[b] = static_cast<uint8_t>(byte);
      for (size_t i = 0; i < kBlockElems; ++i) {
        codes[b * kBlockElems + i] = E4m3Encode(Clamp448(x[i] * inv));
      }
    }
  }
}

// dst[0, n) <- D(packed) (* alpha when alpha != 1: one fp32 multiply)
inline void MxDequantizeHost(const uint8_t* packed, size_t n, float* dst, float alpha = 1.0f) {
  for (size_t i = 0; i < n; ++i) {
    const uint8_t* scales = packed + (i / kSuperElems) * kSuperBytes;
    size_t in_sb = i % kSuperElems;
    int byte = scales[in_sb / kBlockElems];
    float v = std::ldexp(E4m3Decode(scales[kSuperScales + in_sb]), byte - 127);
    dst[i] = alpha == 1.0f ? v : v * alpha;
  }
}

}  // namespace mx
}  // namespace xps
