// Fused shifted-window attention (Swin) for gfx950 (CDNA4): forward and
// backward, bf16 and fp16.  Window 7x7 (S = 49 tokens, padded to 64), head dim
// 32, relative-position bias and the shifted-window region mask.
//
//   qkv  [N, H, W, 3*heads*32]   last dim ordered [3][heads][32]
//   bias [169, heads] fp32       row (dy+6)*13 + (dx+6), d = query - key
//   out  [N, H, W, heads*32]     in the image layout (un-partitioned, unshifted)
//
// Window (wy, wx) token t = 7*i + j is image pixel ((7*wy + i + shift) mod H,
// (7*wx + j + shift) mod W): roll by -shift, partition.  The roll, the
// partition, the head split and their inverses exist only as the per-lane
// source address of a global_load_lds and the per-lane address of a store.
// No score, probability or mask tensor ever reaches memory.
//
// Unit of work: ONE WAVE per (sample, window, head).  A 49-token sequence is
// a single 64x64 score tile, so there is nothing to tile over S and nothing to
// share between waves: the waves of a workgroup never synchronise while they
// work (the backward meets once, at the end, to sum its dbias partials).
//
// Every product is formed TRANSPOSED, so that a lane of the accumulator owns
// one token (column = lane & 31) and its registers run over the other index:
//   S^T  = K Q^T    lane = query, registers = keys: the softmax max / sum are
//                   in-register loops plus ONE cross-lane step (lane ^ 32), and
//                   1/sum is a per-lane scalar of the O^T epilogue
//   O^T  = V^T P^T  lane = query, registers = 4 consecutive head-dim elements:
//                   the result goes to memory as 8-byte stores, written once
//   dP^T = V dO^T, dV^T = dO^T P, dQ^T = K^T dS^T, dK^T = Q^T dS   likewise
// All on mfma_f32_32x32x16 (operands A[lane&31][(lane>>5)*8+e], B alike;
// accumulator register r = row (r&3) + 8*(r>>2) + 4*(lane>>5), column lane&31).
//
// LDS, per wave.  Token images are [64][32] (64-B rows, 4 KiB); rows 49..63
// repeat token 48 (finite data; P and dS are zeroed there, so they contribute
// exactly nothing).  Two copies where both read styles are needed, as the
// notes at the top of attention.hip advise:
//   "s" images  read with b128: 16-B chunk c of row r is stored at chunk
//               c ^ ((r >> 1) & 3), applied to the global SOURCE address.
//               With 64-B rows, rows r and r+2 start on the same bank; the
//               key spreads 8 consecutive rows over all 32 banks.
//   "n" images  natural; read through ds_read_b64_tr_b16 (transposed operand)
//   P / dS tile [64 q][64 k] (128-B rows, 8 KiB): chunk ^ (q & 7) where it is
//               read with b128, natural where it is read through tr.
//   forward : Qs Ks | Vn                  P overlays Qs+Ks      12 KiB
//   backward: Ks Qs | Vs dOs | Kn Qn dOn  P/dSn overlay Ks+Qs,
//                                         dSs overlays Vs+dOs   28 KiB
// plus the head's 169 biases (fp32) and one word per token (its b = 13*i + j
// and its mask region).
//
// dbias: within a unit, bin (dy, dx) is the sum of dS over a fixed set of at
// most 49 (query, key) pairs.  Lane l owns bins l, l+64, l+128 and walks their
// pairs in the dS tile in a fixed order, into registers that live across all
// of the wave's units.  A workgroup handles one head; its waves' partials are
// summed in wave order into ws[block][head][169], and a second kernel sums the
// blocks in a fixed order.  No atomics anywhere; two runs agree bit for bit.
//
// Nothing synchronises with the host and every allocation has a size known
// from the shapes, so all of it can be captured into a hipGraph.

#include <torch/extension.h>

#include <algorithm>
#include <cstdint>

#include "common.h"
#include "dispatch.h"

namespace wattn {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef short v4s __attribute__((ext_vector_type(4)));

template <typename T16>
struct MM;
template <>
struct MM<bf16> {
  using vec = bf16x8;
  DEV_INLINE static f32x16 mma32(vec a, vec b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
  }
  DEV_INLINE static short bits(float v) { return f2bfbits(v); }
};
template <>
struct MM<_Float16> {
  using vec = f16x8;
  DEV_INLINE static f32x16 mma32(vec a, vec b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
  }
  DEV_INLINE static short bits(float v) {
    union {
      _Float16 h;
      short s;
    } u;
    u.h = (_Float16)v;
    return u.s;
  }
};

constexpr int kWin = 7;             // window side
constexpr int kS = kWin * kWin;     // 49 tokens
constexpr int kSP = 64;             // padded tokens
constexpr int kDh = 32;             // head dim
constexpr int kBins = 13 * 13;      // relative-position bins
constexpr int kImg = kSP * kDh;     // elements of a token image (4 KiB)
constexpr int kFwdWaves = 4;        // units per forward workgroup
constexpr int kBwdWaves = 2;        // waves per backward workgroup (LDS bound)
constexpr int kBwdBlockCap = 2048;  // backward workgroups over all heads
constexpr float kMaskValue = -100.f;
constexpr float kNegBig = -3.0e38f;

// bytes of LDS per wave: images, then bias [169] f32 and meta [64] i32
constexpr int kAuxB = 176 * 4 + kSP * 4;
constexpr int kFwdWaveB = 3 * kImg * 2 + kAuxB;
constexpr int kBwdWaveB = 7 * kImg * 2 + kAuxB;
static_assert(kFwdWaveB % 16 == 0 && kBwdWaveB % 16 == 0, "16-B wave slabs");
static_assert(kBwdWaves * kBwdWaveB <= 65536, "backward LDS budget");

#define LDSB(p)                                               \
  ((unsigned)(unsigned long long)(__attribute__((            \
      address_space(3))) const void*)(p))

DEV_INLINE int div7(int t) { return (t * 37) >> 8; }  // exact for 0 <= t < 64

// The window's geometry as one lane sees it.
struct Win {
  int n, wy, wx, H, W, shift;
  // pixel index (n*H + y)*W + x of window token t (t < 49)
  DEV_INLINE long long pixel(int t) const {
    const int i = div7(t), j = t - 7 * i;
    int y = kWin * wy + i + shift, x = kWin * wx + j + shift;
    y -= y >= H ? H : 0;
    x -= x >= W ? W : 0;
    return ((long long)n * H + y) * W + x;
  }
  // b = 13*i + j in bits 0..7, the mask region 3*r(y') + r(x') in bits 8..11
  DEV_INLINE int meta(int t) const {
    const int i = div7(t), j = t - 7 * i;
    int reg = 0;
    if (shift > 0) {
      const int ys = kWin * wy + i, xs = kWin * wx + j;
      const int ry = ys < H - kWin ? 0 : (ys < H - shift ? 1 : 2);
      const int rx = xs < W - kWin ? 0 : (xs < W - shift ? 1 : 2);
      reg = 3 * ry + rx;
    }
    return (13 * i + j) | (reg << 8);
  }
};

// Stage one [64][32] token image: 4 global_load_lds of 1 KiB (16 rows).  Lane
// l brings chunk (l & 3) of LDS row 16*u + (l >> 2); `pix` holds that row's
// pixel for u = 0..3, `col` the element offset of the head's slice inside a
// pixel's channels.  SWZ: fetch the chunk that belongs at this position of a
// chunk-swizzled image.
template <typename T16, bool SWZ>
DEV_INLINE void stage_image(T16* lds, const T16* __restrict__ src,
                            const long long* pix, long long pstride, int col,
                            int lane) {
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int row = 16 * u + (lane >> 2);
    const int c = SWZ ? ((lane & 3) ^ ((row >> 1) & 3)) : (lane & 3);
    const T16* p = src + pix[u] * pstride + col + c * 8;
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) unsigned int*)p,
        (__attribute__((address_space(3))) unsigned int*)(lds + u * 16 * kDh),
        16, 0, 0);
  }
}

// b128 operand from a chunk-swizzled token image: IMG[row][c*8 .. c*8+7]
template <typename T16>
DEV_INLINE typename MM<T16>::vec sw_frag(const T16* img, int row, int c) {
  return *reinterpret_cast<const typename MM<T16>::vec*>(
      img + row * kDh + ((c ^ ((row >> 1) & 3)) * 8));
}
// b128 operand from the chunk-swizzled tile: T[row][c*8 .. c*8+7], c < 8
template <typename T16>
DEV_INLINE typename MM<T16>::vec tile_frag(const T16* tile, int row, int c) {
  return *reinterpret_cast<const typename MM<T16>::vec*>(
      tile + row * kSP + ((c ^ (row & 7)) * 8));
}
// transposed operand from a natural image with rows of STRIDE elements:
// element e of lane l is IMG[sum0 + (l>>5)*8 + e][c0 + (l&31)].  Each group of
// 16 lanes transposes 4 rows x 16 columns; the second read is 4 rows on.
template <typename T16, int STRIDE>
DEV_INLINE typename MM<T16>::vec tr_frag(const T16* img, int sum0, int c0,
                                         int lane) {
  const int row = sum0 + (lane >> 5) * 8 + ((lane & 15) >> 2);
  const int colx = c0 + ((lane >> 4) & 1) * 16 + (lane & 3) * 4;
  const unsigned a = LDSB(img + row * STRIDE + colx);
  v4s l0, h0;
  asm volatile(
      "ds_read_b64_tr_b16 %0, %2 offset:0\n\t"
      "ds_read_b64_tr_b16 %1, %2 offset:%3\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=&v"(l0), "=&v"(h0)
      : "v"(a), "n"(4 * STRIDE * 2)
      : "memory");
  typename MM<T16>::vec b;
  reinterpret_cast<v4s*>(&b)[0] = l0;
  reinterpret_cast<v4s*>(&b)[1] = h0;
  return b;
}

// everything staged by this wave's global_load_lds has landed
DEV_INLINE void wait_staged() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
// this wave's LDS reads and writes are done (before LDS is staged over)
DEV_INLINE void wait_lds() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
// keeps the compiler from moving LDS accesses across a change of overlay
DEV_INLINE void lds_fence() { asm volatile("" ::: "memory"); }

// the key index of accumulator register r of key tile km, for this lane
DEV_INLINE int acc_row(int km, int r, int ks) {
  return km * 32 + (r & 3) + 8 * (r >> 2) + 4 * ks;
}

// Scores of the lane's query against the 32 keys it holds (two key tiles):
// s = scale*qk + bias[rel] + mask, kNegBig for padded keys.  qa = the query's
// 13*i + j + 84, qreg its region.  Returns the row max over all 64 keys.
DEV_INLINE float scores(f32x16 (&acc)[2], const float* bias, const int* meta,
                        int qa, int qreg, int ks, float scale) {
  float m = kNegBig;
#pragma unroll
  for (int km = 0; km < 2; ++km)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int k = acc_row(km, r, ks);
      float s = kNegBig;
      if (k < kS) {
        const int mk = meta[k];
        s = acc[km][r] * scale + bias[qa - (mk & 0xff)];
        s += (mk >> 8) != qreg ? kMaskValue : 0.f;
      }
      acc[km][r] = s;
      m = fmaxf(m, s);
    }
  return fmaxf(m, __shfl_xor(m, 32));
}

// 4 consecutive head-dim elements of one token to memory (8 bytes)
template <typename T16>
DEV_INLINE void store4(T16* dst, float a, float b, float c, float d) {
  v4s v;
  v[0] = MM<T16>::bits(a);
  v[1] = MM<T16>::bits(b);
  v[2] = MM<T16>::bits(c);
  v[3] = MM<T16>::bits(d);
  *reinterpret_cast<v4s*>(dst) = v;
}

// accumulator of a transposed [32 d][32 tokens] product -> the token's 64-B
// slice at dst: register group g holds d = 8g + 4ks .. +3
template <typename T16>
DEV_INLINE void store_slice(T16* dst, const f32x16& acc, float f, int ks) {
#pragma unroll
  for (int g = 0; g < 4; ++g)
    store4<T16>(dst + 8 * g + 4 * ks, acc[4 * g] * f, acc[4 * g + 1] * f,
                acc[4 * g + 2] * f, acc[4 * g + 3] * f);
}

// =============================== forward ==================================

template <typename T16>
__global__ __launch_bounds__(kFwdWaves * 64) void fwd_kernel(
    const T16* __restrict__ qkv, const float* __restrict__ bias_table,
    T16* __restrict__ out, int H, int W, int heads, int shift, float scale,
    long long units) {
  __shared__ __attribute__((aligned(16))) char smem[kFwdWaves * kFwdWaveB];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long unit = (long long)blockIdx.x * kFwdWaves + wave;
  if (unit >= units) return;  // tail: no barrier below, the wave just leaves
  T16* Qs = reinterpret_cast<T16*>(smem + wave * kFwdWaveB);
  T16* Ks = Qs + kImg;
  T16* Vn = Ks + kImg;
  T16* Pt = Qs;  // overlays Qs + Ks once S^T is in registers
  float* bias = reinterpret_cast<float*>(Vn + kImg);
  int* meta = reinterpret_cast<int*>(bias + 176);

  using vec16 = typename MM<T16>::vec;
  const int nwx = W / kWin, nw = (H / kWin) * nwx;
  const int head = (int)(unit % heads);
  const long long rest = unit / heads;
  const int w = (int)(rest % nw);
  const Win win{(int)(rest / nw), w / nwx, w % nwx, H, W, shift};
  const int C = heads * kDh;
  const int r32 = lane & 31, ks = lane >> 5;

  long long pix[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) pix[u] = win.pixel(min(16 * u + (lane >> 2), kS - 1));
  stage_image<T16, true>(Qs, qkv, pix, 3LL * C, head * kDh, lane);
  stage_image<T16, true>(Ks, qkv, pix, 3LL * C, C + head * kDh, lane);
  stage_image<T16, false>(Vn, qkv, pix, 3LL * C, 2 * C + head * kDh, lane);
  for (int b = lane; b < kBins; b += 64) bias[b] = bias_table[b * heads + head];
  meta[lane] = win.meta(min(lane, kS - 1));
  wait_staged();

  // the lane's two queries (one per query tile)
  int qtok[2], qa[2], qreg[2];
#pragma unroll
  for (int qn = 0; qn < 2; ++qn) {
    qtok[qn] = qn * 32 + r32;
    const int mq = meta[min(qtok[qn], kS - 1)];
    qa[qn] = (mq & 0xff) + 84;
    qreg[qn] = mq >> 8;
  }

  // ---- S^T = K Q^T: acc[qn][km], rows = keys, column = the lane's query ----
  f32x16 acc[2][2] = {};
#pragma unroll
  for (int kc = 0; kc < 2; ++kc) {
    vec16 a[2], b[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      a[t] = sw_frag<T16>(Ks, t * 32 + r32, kc * 2 + ks);
      b[t] = sw_frag<T16>(Qs, t * 32 + r32, kc * 2 + ks);
    }
#pragma unroll
    for (int qn = 0; qn < 2; ++qn)
#pragma unroll
      for (int km = 0; km < 2; ++km)
        acc[qn][km] = MM<T16>::mma32(a[km], b[qn], acc[qn][km]);
  }
  lds_fence();  // Qs / Ks are dead: P may overlay them

  // ---- softmax in registers; exp (un-normalised) -> P tile [q][k] ----
  float inv[2];
#pragma unroll
  for (int qn = 0; qn < 2; ++qn) {
    const float m = scores(acc[qn], bias, meta, qa[qn], qreg[qn], ks, scale);
    float sum = 0.f;
    const int q = qtok[qn];
#pragma unroll
    for (int km = 0; km < 2; ++km)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        v4s pk;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int k = acc_row(km, 4 * g + e, ks);
          const float p = k < kS ? __expf(acc[qn][km][4 * g + e] - m) : 0.f;
          pk[e] = MM<T16>::bits(p);
          sum += p;
        }
        const int c = km * 4 + g;  // 16-B chunk of keys; ks picks its half
        *reinterpret_cast<v4s*>(Pt + q * kSP + ((c ^ (q & 7)) * 8) + ks * 4) =
            pk;
      }
    sum += __shfl_xor(sum, 32);
    inv[qn] = 1.f / sum;
  }
  lds_fence();

  // ---- O^T = V^T P^T: rows = head dim, column = the lane's query ----
  f32x16 o[2] = {};
#pragma unroll
  for (int kc = 0; kc < 4; ++kc) {
    const vec16 a = tr_frag<T16, kDh>(Vn, kc * 16, 0, lane);
#pragma unroll
    for (int qn = 0; qn < 2; ++qn) {
      const vec16 b = tile_frag<T16>(Pt, qn * 32 + r32, kc * 2 + ks);
      o[qn] = MM<T16>::mma32(a, b, o[qn]);
    }
  }
#pragma unroll
  for (int qn = 0; qn < 2; ++qn)
    if (qtok[qn] < kS)
      store_slice<T16>(out + win.pixel(qtok[qn]) * C + head * kDh, o[qn],
                       inv[qn], ks);
}

// =============================== backward =================================

template <typename T16>
__global__ __launch_bounds__(kBwdWaves * 64) void bwd_kernel(
    const T16* __restrict__ dout, const T16* __restrict__ qkv,
    const float* __restrict__ bias_table, T16* __restrict__ dqkv,
    float* __restrict__ ws, int H, int W, int heads, int shift, float scale,
    int nunits) {
  __shared__ __attribute__((aligned(16))) char smem[kBwdWaves * kBwdWaveB];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  T16* Ks = reinterpret_cast<T16*>(smem + wave * kBwdWaveB);
  T16* Qs = Ks + kImg;
  T16* Vs = Qs + kImg;
  T16* Os = Vs + kImg;
  T16* Kn = Os + kImg;
  T16* Qn = Kn + kImg;
  T16* On = Qn + kImg;
  T16* Pn = Ks;   // P, then dS, natural [q][k]; overlays Ks + Qs
  T16* Ss = Vs;   // dS chunk-swizzled;          overlays Vs + dOs
  float* bias = reinterpret_cast<float*>(On + kImg);
  int* meta = reinterpret_cast<int*>(bias + 176);

  using vec16 = typename MM<T16>::vec;
  const int head = blockIdx.y;
  const int nwx = W / kWin, nw = (H / kWin) * nwx;
  const int C = heads * kDh;
  const int r32 = lane & 31, ks = lane >> 5;

  for (int b = lane; b < kBins; b += 64) bias[b] = bias_table[b * heads + head];

  // sums of the bins this lane owns (b = lane + 64*p) over the wave's units
  float dbacc[3] = {0.f, 0.f, 0.f};

  for (int u = blockIdx.x * kBwdWaves + wave; u < nunits;
       u += gridDim.x * kBwdWaves) {
    const int w = u % nw;
    const Win win{u / nw, w / nwx, w % nwx, H, W, shift};
    long long pix[4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
      pix[t] = win.pixel(min(16 * t + (lane >> 2), kS - 1));
    wait_lds();  // the previous unit's reads are done before LDS is re-staged
    const int hc = head * kDh;
    stage_image<T16, true>(Ks, qkv, pix, 3LL * C, C + hc, lane);
    stage_image<T16, true>(Qs, qkv, pix, 3LL * C, hc, lane);
    stage_image<T16, true>(Vs, qkv, pix, 3LL * C, 2 * C + hc, lane);
    stage_image<T16, true>(Os, dout, pix, C, hc, lane);
    stage_image<T16, false>(Kn, qkv, pix, 3LL * C, C + hc, lane);
    stage_image<T16, false>(Qn, qkv, pix, 3LL * C, hc, lane);
    stage_image<T16, false>(On, dout, pix, C, hc, lane);
    meta[lane] = win.meta(min(lane, kS - 1));
    wait_staged();

    int qtok[2], qa[2], qreg[2];
    long long qpix[2];
#pragma unroll
    for (int qn = 0; qn < 2; ++qn) {
      qtok[qn] = qn * 32 + r32;
      const int mq = meta[min(qtok[qn], kS - 1)];
      qa[qn] = (mq & 0xff) + 84;
      qreg[qn] = mq >> 8;
      qpix[qn] = win.pixel(min(qtok[qn], kS - 1));
    }

    // ---- S^T = K Q^T and dP^T = V dO^T: rows = keys, column = query ----
    f32x16 acc[2][2] = {}, dp[2][2] = {};
#pragma unroll
    for (int kc = 0; kc < 2; ++kc) {
      vec16 a[2], b[2], av[2], bo[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        a[t] = sw_frag<T16>(Ks, t * 32 + r32, kc * 2 + ks);
        b[t] = sw_frag<T16>(Qs, t * 32 + r32, kc * 2 + ks);
        av[t] = sw_frag<T16>(Vs, t * 32 + r32, kc * 2 + ks);
        bo[t] = sw_frag<T16>(Os, t * 32 + r32, kc * 2 + ks);
      }
#pragma unroll
      for (int qn = 0; qn < 2; ++qn)
#pragma unroll
        for (int km = 0; km < 2; ++km) {
          acc[qn][km] = MM<T16>::mma32(a[km], b[qn], acc[qn][km]);
          dp[qn][km] = MM<T16>::mma32(av[km], bo[qn], dp[qn][km]);
        }
    }
    lds_fence();  // the four "s" images are dead: the tiles overlay them

    // ---- P (recomputed) and dS = P o (dP - D), D = sum_k P dP ----
    // P -> Pn; dS -> Ss now, and kept in dp for Pn after dV has read P
#pragma unroll
    for (int qn = 0; qn < 2; ++qn) {
      const int q = qtok[qn];
      const float m = scores(acc[qn], bias, meta, qa[qn], qreg[qn], ks, scale);
      float sum = 0.f;
#pragma unroll
      for (int km = 0; km < 2; ++km)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float p =
              acc_row(km, r, ks) < kS ? __expf(acc[qn][km][r] - m) : 0.f;
          acc[qn][km][r] = p;
          sum += p;
        }
      sum += __shfl_xor(sum, 32);
      // a padded query row holds nothing: P = dS = 0 there
      const float rs = q < kS ? 1.f / sum : 0.f;
      float D = 0.f;
#pragma unroll
      for (int km = 0; km < 2; ++km)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          acc[qn][km][r] *= rs;
          D += acc[qn][km][r] * dp[qn][km][r];
        }
      D += __shfl_xor(D, 32);
#pragma unroll
      for (int km = 0; km < 2; ++km)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          v4s pk, sk;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int r = 4 * g + e;
            const float p = acc[qn][km][r];
            const float ds = p * (dp[qn][km][r] - D);
            pk[e] = MM<T16>::bits(p);
            sk[e] = MM<T16>::bits(ds);
            dp[qn][km][r] = ds;  // waits here for its natural copy
          }
          const int c = km * 4 + g;
          *reinterpret_cast<v4s*>(Pn + q * kSP + c * 8 + ks * 4) = pk;
          *reinterpret_cast<v4s*>(Ss + q * kSP + ((c ^ (q & 7)) * 8) +
                                  ks * 4) = sk;
        }
    }
    lds_fence();

    // ---- dV^T = dO^T P and dQ^T = K^T dS^T ----
    f32x16 dv[2] = {}, dq[2] = {};
#pragma unroll
    for (int kc = 0; kc < 4; ++kc) {
      const vec16 ao = tr_frag<T16, kDh>(On, kc * 16, 0, lane);
      const vec16 ak = tr_frag<T16, kDh>(Kn, kc * 16, 0, lane);
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const vec16 bp = tr_frag<T16, kSP>(Pn, kc * 16, t * 32, lane);
        const vec16 bs = tile_frag<T16>(Ss, t * 32 + r32, kc * 2 + ks);
        dv[t] = MM<T16>::mma32(ao, bp, dv[t]);
        dq[t] = MM<T16>::mma32(ak, bs, dq[t]);
      }
    }
    lds_fence();  // P has been read: dS (natural) takes its place
#pragma unroll
    for (int qn = 0; qn < 2; ++qn)
#pragma unroll
      for (int km = 0; km < 2; ++km)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          v4s sk;
#pragma unroll
          for (int e = 0; e < 4; ++e)
            sk[e] = MM<T16>::bits(dp[qn][km][4 * g + e]);
          *reinterpret_cast<v4s*>(Pn + qtok[qn] * kSP + (km * 4 + g) * 8 +
                                  ks * 4) = sk;
        }
    lds_fence();

    // ---- dK^T = Q^T dS ----
    f32x16 dk[2] = {};
#pragma unroll
    for (int kc = 0; kc < 4; ++kc) {
      const vec16 aq = tr_frag<T16, kDh>(Qn, kc * 16, 0, lane);
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const vec16 bs = tr_frag<T16, kSP>(Pn, kc * 16, t * 32, lane);
        dk[t] = MM<T16>::mma32(aq, bs, dk[t]);
      }
    }

    // ---- dqkv: the lane's token (t*32 + r32) gets its q, k and v slices ----
#pragma unroll
    for (int t = 0; t < 2; ++t)
      if (qtok[t] < kS) {
        T16* dst = dqkv + qpix[t] * 3LL * C + hc;
        store_slice<T16>(dst, dq[t], scale, ks);
        store_slice<T16>(dst + C, dk[t], scale, ks);
        store_slice<T16>(dst + 2 * C, dv[t], 1.f, ks);
      }

    // ---- dbias: each lane walks the pairs of its bins in the dS tile ----
#pragma unroll
    for (int p = 0; p < 3; ++p) {
      const int b = lane + 64 * p;
      if (b < kBins) {
        const int dy = b / 13 - 6, dx = b % 13 - 6;
        const int i0 = max(0, dy), i1 = min(6, 6 + dy);
        const int j0 = max(0, dx), j1 = min(6, 6 + dx);
        float s = 0.f;
        for (int qi = i0; qi <= i1; ++qi)
          for (int qj = j0; qj <= j1; ++qj)
            s += to_f<T16>(Pn[(qi * 7 + qj) * kSP + (qi - dy) * 7 + (qj - dx)]);
        dbacc[p] += s;
      }
    }
  }

  // ---- the workgroup's partial: waves summed in order ----
  __syncthreads();  // every wave is done with its LDS
  float* red = reinterpret_cast<float*>(smem);  // [waves][192]
#pragma unroll
  for (int p = 0; p < 3; ++p) red[wave * 192 + lane + 64 * p] = dbacc[p];
  __syncthreads();
  for (int b = threadIdx.x; b < kBins; b += kBwdWaves * 64) {
    float s = 0.f;
#pragma unroll
    for (int wv = 0; wv < kBwdWaves; ++wv) s += red[wv * 192 + b];
    ws[((long long)blockIdx.x * heads + head) * kBins + b] = s;
  }
}

// ws [nb][heads][169] -> dbias [169][heads]: one thread per output; four
// interleaved running sums over the blocks, combined in a fixed order.
__global__ __launch_bounds__(256) void dbias_reduce_kernel(
    const float* __restrict__ ws, float* __restrict__ dbias, int nb,
    int heads) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= kBins * heads) return;
  const int b = i / heads, h = i - b * heads;
  const float* p = ws + (long long)h * kBins + b;
  const long long stride = (long long)heads * kBins;
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  int blk = 0;
  for (; blk + 4 <= nb; blk += 4) {
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] += p[(blk + k) * stride];
  }
  for (int k = 0; blk < nb; ++blk, ++k) s[k] += p[blk * stride];
  dbias[i] = (s[0] + s[1]) + (s[2] + s[3]);
}

#undef LDSB

}  // namespace wattn

// ======================= host launchers ==================================

namespace {

struct WinShape {
  int N, H, W, heads, shift;
};

WinShape check_win(const char* name, const torch::Tensor& qkv,
                   const torch::Tensor& bias_table, int64_t heads,
                   int64_t shift) {
  TORCH_CHECK(qkv.is_cuda() && qkv.dim() == 4 && qkv.is_contiguous(), name,
              ": qkv must be a contiguous [N,H,W,3*heads*32] GPU tensor");
  TORCH_CHECK(qkv.scalar_type() == torch::kBFloat16 ||
                  qkv.scalar_type() == torch::kHalf,
              name, ": bf16/f16 only");
  TORCH_CHECK(heads >= 1 && heads <= 65535, name,
              ": heads must be in [1, 65535], got ", heads);
  TORCH_CHECK(qkv.size(3) == 3 * heads * wattn::kDh, name,
              ": the head dim must be 32 (channels = 3*heads*32), got ",
              qkv.size(3), " channels for ", heads, " heads");
  TORCH_CHECK(qkv.size(1) >= 7 && qkv.size(1) % 7 == 0 && qkv.size(2) >= 7 &&
                  qkv.size(2) % 7 == 0,
              name, ": H and W must be multiples of the window size 7, got ",
              qkv.size(1), "x", qkv.size(2));
  TORCH_CHECK(shift >= 0 && shift < 7, name,
              ": shift must be in [0, 7), got ", shift);
  TORCH_CHECK(qkv.size(0) >= 1, name, ": empty batch");
  TORCH_CHECK((reinterpret_cast<uintptr_t>(qkv.data_ptr()) & 15u) == 0, name,
              ": tensors must be 16-byte aligned");
  TORCH_CHECK(bias_table.is_cuda() && bias_table.device() == qkv.device() &&
                  bias_table.dim() == 2 &&
                  bias_table.size(0) == wattn::kBins &&
                  bias_table.size(1) == heads,
              name, ": bias_table must be [169, heads] on qkv's device");
  TORCH_CHECK(bias_table.scalar_type() == torch::kFloat32 ||
                  bias_table.scalar_type() == qkv.scalar_type(),
              name, ": bias_table must be fp32 or qkv's dtype");
  const long long units =
      (long long)qkv.size(0) * (qkv.size(1) / 7) * (qkv.size(2) / 7);
  TORCH_CHECK(units * heads <= 0x7fffffffLL, name, ": too many windows");
  return WinShape{(int)qkv.size(0), (int)qkv.size(1), (int)qkv.size(2),
                  (int)heads, (int)shift};
}

}  // namespace

torch::Tensor win_attn_fwd(torch::Tensor qkv, torch::Tensor bias_table,
                           int64_t heads, int64_t shift, double scale) {
  const WinShape s = check_win("win_attn_fwd", qkv, bias_table, heads, shift);
  auto bias = bias_table.to(torch::kFloat32).contiguous();
  auto out = torch::empty({s.N, s.H, s.W, s.heads * wattn::kDh}, qkv.options());
  const long long units = (long long)s.N * (s.H / 7) * (s.W / 7) * s.heads;
  const unsigned grid =
      (unsigned)((units + wattn::kFwdWaves - 1) / wattn::kFwdWaves);
  dispatch16(qkv, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL((wattn::fwd_kernel<T>), dim3(grid),
                       dim3(wattn::kFwdWaves * 64), 0,
                       c10::hip::getCurrentHIPStream(), ptr16<const T>(qkv),
                       bias.data_ptr<float>(), ptr16<T>(out), s.H, s.W,
                       s.heads, s.shift, (float)scale, units);
  });
  return out;
}

std::vector<torch::Tensor> win_attn_bwd(torch::Tensor dout, torch::Tensor qkv,
                                        torch::Tensor bias_table,
                                        int64_t heads, int64_t shift,
                                        double scale) {
  const WinShape s = check_win("win_attn_bwd", qkv, bias_table, heads, shift);
  TORCH_CHECK(dout.is_cuda() && dout.is_contiguous() && dout.dim() == 4 &&
                  dout.scalar_type() == qkv.scalar_type() &&
                  dout.device() == qkv.device() && dout.size(0) == s.N &&
                  dout.size(1) == s.H && dout.size(2) == s.W &&
                  dout.size(3) == s.heads * wattn::kDh,
              "win_attn_bwd: dout must be a contiguous [N,H,W,heads*32] "
              "tensor of qkv's dtype");
  TORCH_CHECK((reinterpret_cast<uintptr_t>(dout.data_ptr()) & 15u) == 0,
              "win_attn_bwd: tensors must be 16-byte aligned");
  auto bias = bias_table.to(torch::kFloat32).contiguous();
  auto dqkv = torch::empty_like(qkv);
  const int nunits = s.N * (s.H / 7) * (s.W / 7);  // per head
  const int nb = std::min(
      (nunits + wattn::kBwdWaves - 1) / wattn::kBwdWaves,
      std::max(1, wattn::kBwdBlockCap / s.heads));
  auto fopt = qkv.options().dtype(torch::kFloat32);
  auto ws = torch::empty({nb, s.heads, wattn::kBins}, fopt);
  auto dbias = torch::empty({wattn::kBins, s.heads}, fopt);
  auto stream = c10::hip::getCurrentHIPStream();
  dispatch16(qkv, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL((wattn::bwd_kernel<T>), dim3(nb, s.heads),
                       dim3(wattn::kBwdWaves * 64), 0, stream,
                       ptr16<const T>(dout), ptr16<const T>(qkv),
                       bias.data_ptr<float>(), ptr16<T>(dqkv),
                       ws.data_ptr<float>(), s.H, s.W, s.heads, s.shift,
                       (float)scale, nunits);
  });
  hipLaunchKernelGGL(wattn::dbias_reduce_kernel,
                     dim3((wattn::kBins * s.heads + 255) / 256), dim3(256), 0,
                     stream, ws.data_ptr<float>(), dbias.data_ptr<float>(), nb,
                     s.heads);
  return {dqkv, dbias};
}
