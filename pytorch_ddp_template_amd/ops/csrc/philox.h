// Philox4x32-10 and the attention-probability keep mask built on it: the one
// device copy shared by dropout.hip and attention.hip (ops/rng.py mirrors
// both in numpy).
#pragma once

#include <cstdint>

#include "common.h"

namespace rng {

constexpr uint32_t kMul0 = 0xD2511F53u, kMul1 = 0xCD9E8D57u;
constexpr uint32_t kWeyl0 = 0x9E3779B9u, kWeyl1 = 0xBB67AE85u;

struct U4 {
  uint32_t w0, w1, w2, w3;
};

// Philox4x32-10.  The two 32x32 -> 64 products per round are plain C++; the
// compiler picks the multiply instructions.
DEV_INLINE U4 philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                     uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)kMul0 * c0;
    const uint64_t p1 = (uint64_t)kMul1 * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += kWeyl0;
    k1 += kWeyl1;
  }
  return {c0, c1, c2, c3};
}

// ---- attention-probability dropout: one byte per element ----------------
//
// Element (bh, q, k) of the [B, S, S] probabilities, with rho = q & 31,
// ks = (rho >> 2) & 1 and j = (rho & 3) + 4 * (rho >> 3), draws byte j of the
// block whose counter is
//   (((bh * ceil(S/32) + (q >> 5)) * 2 + ks) * S + k, call lo, call hi, step)
// and is kept iff byte >= thr8 = floor(p * 256), scaled by 256 / (256 - thr8).
// (ks, j) is where the mfma_f32_32x32x16 accumulator keeps row rho: lane
// half ks, register j.  A lane of a 32x32 score quadrant therefore owns
// exactly one block, whatever the tile order, wave or grid around it.
struct AttnDrop {
  const uint32_t* step;  // the device step scalar of ops/rng.py
  uint32_t key0, key1;
  uint32_t cid_lo, cid_hi;
  uint32_t thr8;
  uint32_t nq32;  // ceil(S / 32)
  float scale;
};

// The 16 keep flags of column k in quadrant (bh, q32), lane half ks, packed
// into one register: element j sits at bit 8 * (j & 3) + (j >> 2).
DEV_INLINE uint32_t attn_keep_bits(const AttnDrop& d, uint32_t step,
                                   uint32_t bh, uint32_t q32, uint32_t ks,
                                   uint32_t S, uint32_t k) {
  const uint32_t c0 = ((bh * d.nq32 + q32) * 2 + ks) * S + k;
  const U4 w = philox(c0, d.cid_lo, d.cid_hi, step, d.key0, d.key1);
  // byte >= thr8 for the four bytes of a word at once: bit 7 of
  // (x & 0x7f) + (0x80 - (thr8 & 0x7f)) says whether the low seven bits
  // reach the threshold's (no carry leaves a byte); the top bits decide
  // first: with thr8 < 128 a set top bit is enough, else it is required.
  const uint32_t add = (0x80u - (d.thr8 & 0x7fu)) * 0x01010101u;
  const bool hi = d.thr8 >= 0x80u;
  auto ge = [&](uint32_t x) {
    const uint32_t s = (x & 0x7f7f7f7fu) + add;
    return (hi ? (x & s) : (x | s)) & 0x80808080u;
  };
  return (ge(w.w0) >> 7) | (ge(w.w1) >> 6) | (ge(w.w2) >> 5) | (ge(w.w3) >> 4);
}

// v if element j of `bits` is kept, else +0 (a select on the bit pattern)
DEV_INLINE float attn_keep(uint32_t bits, int j, float v) {
  const int bit = 8 * (j & 3) + (j >> 2);
  const uint32_t m = (uint32_t)((int32_t)(bits << (31 - bit)) >> 31);
  return __uint_as_float(__float_as_uint(v) & m);
}

}  // namespace rng
