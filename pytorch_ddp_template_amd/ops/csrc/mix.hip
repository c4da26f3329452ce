// Mixup / cutmix on the device (CDNA4, gfx950): a draw kernel that writes the
// step's mixing parameters and a batch-mix kernel that applies them in place.
//
// Nothing comes from the host: a captured training step replays both kernels,
// the draw reads the live step scalar of ops/rng.py, and every replay mixes
// with a fresh lambda and box.  The soft-target loss (loss.hip) reads the
// label weight from the same record.
//
// ---- the record ("mix params"): 8 four-byte slots ------------------------
//   0  lam  f32  label weight of the sample's own label
//   1  a    f32  blend weight: lam for mixup, 1 for cutmix / not applied
//   2  y0   i32 \  cutmix box [y0, y1) x [x0, x1); empty (all 0) for mixup
//   3  y1   i32 |  and when not applied
//   4  x0   i32 |
//   5  x1   i32 /
//   6  mode i32  0 not applied, 1 mixup, 2 cutmix
//   7  raw  f32  lambda as drawn, before the box correction (not read by any
//                kernel; kept for tests and logging)
//
// ---- the draw: one wave ---------------------------------------------------
// Philox4x32-10 under (key0, key1), counters (c0, call lo, call hi, step):
//   c0 = 64      choice block: w0 < floor(prob * 2^32) -> apply,
//                w1 < floor(switch * 2^32) -> cutmix (forced when only one
//                alpha is nonzero), cy = w2 mod H, cx = w3 mod W
//   c0 = t < 64  try t of Joehnk's Beta(alpha, alpha) sampler, one per lane:
//                U = (w0 + 0.5) 2^-32, V = (w1 + 0.5) 2^-32,
//                X = U^(1/alpha), Y = V^(1/alpha), accept iff X + Y <= 1
// The lowest accepting lane wins (ballot + find-first) and lambda =
// X / (X + Y) is read from it with a shuffle: a rejection loop turned into
// one wave-wide step.  For alpha <= 1 a try accepts with probability >= 1/2,
// so "no lane accepts" (lambda = 0.5) has probability <= 2^-64.  The box is
// timm's: r = sqrt(1 - lambda), ch = (int)(H r), cw = (int)(W r), corners
// clamped to the image, and the label weight becomes the exact share of the
// image that survives.  ops/rng.py mix_draw mirrors every step in float64.
//
// ---- the batch mix --------------------------------------------------------
// The partner of sample i is B-1-i (timm's batch flip), so a work item is one
// 16-byte vector of one PAIR (p, B-1-p): the thread loads the vector of both
// samples, computes both outputs and stores both.  Every element is read once
// and written once, in place, with no second buffer and no permutation
// tensor.  The middle sample of an odd batch pairs with itself and is skipped.
// Inside the box an element is the partner's, bit for bit; outside it is
// a x + (1 - a) x_partner in fp32, rounded once, or x itself when a == 1 (so
// cutmix only copies).  One box test serves NHWC and NCHW: with row = W * xmul
// (xmul = C for NHWC, 1 for NCHW) element e of a sample lies at
// h = (e / row) % H, xr = e % row, inside iff y0 <= h < y1 and
// x0 * xmul <= xr < x1 * xmul; (h, xr) is divided out once per vector and
// stepped per element, so a vector may straddle pixels, rows and box edges.

#include <torch/extension.h>

#include <cmath>
#include <cstdint>

#include "common.h"
#include "dispatch.h"
#include "philox.h"

namespace mix {

constexpr int kBlock = 256;
constexpr int kGridCap = 2048;
constexpr int kSlots = 8;

struct DrawArgs {
  uint32_t key0, key1;
  uint32_t cid_lo, cid_hi;
  unsigned long long thr_apply, thr_cut;  // floor(p * 2^32): may be 2^32
  int H, W;
  float inv_mix, inv_cut;  // 1 / alpha, 0 when that mode is off
};

// U^(1/alpha) for U = (w + 0.5) 2^-32
DEV_INLINE float pow_unit(uint32_t w, float inv_alpha) {
  const float u = ((float)w + 0.5f) * 2.3283064365386963e-10f;
  return exp2f(log2f(u) * inv_alpha);
}

DEV_INLINE int clampi(int v, int lo, int hi) {
  return v < lo ? lo : (v > hi ? hi : v);
}

__global__ NO_PK_F32 void draw_kernel(float* __restrict__ rec,
                                      const uint32_t* __restrict__ step_ptr,
                                      DrawArgs d) {
  const uint32_t step = *step_ptr;
  const int lane = lane_id();
  const rng::U4 c =
      rng::philox(64u, d.cid_lo, d.cid_hi, step, d.key0, d.key1);
  const bool apply = (unsigned long long)c.w0 < d.thr_apply;
  const bool cut = d.inv_mix == 0.f
                       ? true
                       : (d.inv_cut == 0.f
                              ? false
                              : (unsigned long long)c.w1 < d.thr_cut);
  const float inv_alpha = cut ? d.inv_cut : d.inv_mix;
  const rng::U4 w =
      rng::philox((uint32_t)lane, d.cid_lo, d.cid_hi, step, d.key0, d.key1);
  const float X = pow_unit(w.w0, inv_alpha);
  const float Y = pow_unit(w.w1, inv_alpha);
  const float s = X + Y;
  const unsigned long long acc = __ballot(s <= 1.0f && s > 0.f);
  float lam = 0.5f, oml = 0.5f;  // oml = 1 - lam, formed without cancellation
  if (acc != 0ull) {
    const int win = __ffsll((long long)acc) - 1;
    const float xs = __shfl(X, win), ys = __shfl(Y, win);
    lam = xs / (xs + ys);
    oml = ys / (xs + ys);
  }
  if (lane != 0) return;
  int* reci = reinterpret_cast<int*>(rec);
  if (!apply) {
    rec[0] = 1.f;
    rec[1] = 1.f;
    reci[2] = reci[3] = reci[4] = reci[5] = 0;
    reci[6] = 0;
    rec[7] = 1.f;
    return;
  }
  rec[7] = lam;
  if (!cut) {
    rec[0] = lam;
    rec[1] = lam;
    reci[2] = reci[3] = reci[4] = reci[5] = 0;
    reci[6] = 1;
    return;
  }
  const int cy = (int)(c.w2 % (uint32_t)d.H);
  const int cx = (int)(c.w3 % (uint32_t)d.W);
  const float r = sqrtf(oml);
  const int ch = (int)((float)d.H * r), cw = (int)((float)d.W * r);
  const int y0 = clampi(cy - ch / 2, 0, d.H), y1 = clampi(cy + ch / 2, 0, d.H);
  const int x0 = clampi(cx - cw / 2, 0, d.W), x1 = clampi(cx + cw / 2, 0, d.W);
  const int hw = d.H * d.W;
  // one correctly rounded division of two exact integers
  rec[0] = (float)(hw - (y1 - y0) * (x1 - x0)) / (float)hw;
  rec[1] = 1.f;
  reci[2] = y0;
  reci[3] = y1;
  reci[4] = x0;
  reci[5] = x1;
  reci[6] = 2;
}

// P elements of T held for one lane: a 16-byte vector or a single element
template <typename T, bool VEC>
struct Pack;

template <typename T>
struct Pack<T, true> {
  using IO = VecIO<T>;
  static constexpr int kN = IO::kPerLane;
  typename IO::Vec v;
  DEV_INLINE void load(const T* p) {
    v = *reinterpret_cast<const typename IO::Vec*>(p);
  }
  DEV_INLINE void store(T* p) const {
    *reinterpret_cast<typename IO::Vec*>(p) = v;
  }
  DEV_INLINE float get(int j) const { return IO::get(v, j); }
  DEV_INLINE void set(int j, float x) { IO::set(v, j, x); }
  DEV_INLINE void copy(int j, const Pack& s) { v[j] = s.v[j]; }  // raw bits
};

template <typename T>
struct Pack<T, false> {
  static constexpr int kN = 1;
  T v;
  DEV_INLINE void load(const T* p) { v = *p; }
  DEV_INLINE void store(T* p) const { *p = v; }
  DEV_INLINE float get(int) const { return to_f(v); }
  DEV_INLINE void set(int, float x) { v = to_t<T>(x); }
  DEV_INLINE void copy(int, const Pack& s) { v = s.v; }
};

struct MixArgs {
  long long work;  // pairs * per
  long long n;     // elements per sample
  uint32_t per;    // packs per sample (n / P)
  uint32_t B;
  uint32_t row;    // W * xmul
  uint32_t H;
  uint32_t xmul;
};

template <typename T, bool VEC>
__global__ NO_PK_F32 void batch_kernel(T* __restrict__ x,
                                       const float* __restrict__ rec,
                                       MixArgs m) {
  using PK = Pack<T, VEC>;
  constexpr int P = PK::kN;
  const int* reci = reinterpret_cast<const int*>(rec);
  if (reci[6] == 0) return;  // not applied: the batch stays as it is
  const float a = rec[1], oma = 1.f - a;
  const bool keep = a == 1.f;
  const uint32_t y0 = (uint32_t)reci[2], y1 = (uint32_t)reci[3];
  const uint32_t xlo = (uint32_t)reci[4] * m.xmul;
  const uint32_t xhi = (uint32_t)reci[5] * m.xmul;
  GRID_STRIDE(i, m.work) {
    // pairs * packs fits 32 bits in every shape the models produce; the
    // 64-bit divide is the long way round
    const uint32_t p = (i >> 32) == 0 ? (uint32_t)i / m.per
                                      : (uint32_t)(i / (long long)m.per);
    const uint32_t v = (uint32_t)(i - (long long)p * m.per);
    const uint32_t q = m.B - 1u - p;
    if (q == p) continue;  // the middle sample of an odd batch
    const uint32_t e0 = v * (uint32_t)P;
    T* pa = x + (long long)p * m.n + e0;
    T* pb = x + (long long)q * m.n + e0;
    PK va, vb, oa, ob;
    va.load(pa);
    vb.load(pb);
    const uint32_t rw = e0 / m.row;
    uint32_t h = rw % m.H, xr = e0 - rw * m.row;
#pragma unroll
    for (int j = 0; j < P; ++j) {
      const bool in = h >= y0 && h < y1 && xr >= xlo && xr < xhi;
      if (in) {
        oa.copy(j, vb);
        ob.copy(j, va);
      } else if (keep) {
        oa.copy(j, va);
        ob.copy(j, vb);
      } else {
        const float fa = va.get(j), fb = vb.get(j);
        oa.set(j, a * fa + oma * fb);
        ob.set(j, a * fb + oma * fa);
      }
      if (++xr == m.row) {
        xr = 0;
        if (++h == m.H) h = 0;
      }
    }
    oa.store(pa);
    ob.store(pb);
  }
}

}  // namespace mix

// ======================= host launchers ==================================

namespace {

inline bool mix_aligned16(const void* p) {
  return (reinterpret_cast<uintptr_t>(p) & 15u) == 0;
}

void check_record(const torch::Tensor& rec, const char* who) {
  TORCH_CHECK(rec.is_cuda() && rec.is_contiguous() &&
                  rec.scalar_type() == torch::kFloat32 &&
                  rec.numel() == mix::kSlots,
              who, ": the mix params must be a contiguous float32 GPU tensor "
              "of 8 slots");
}

inline float inv_alpha(double alpha, const char* name) {
  TORCH_CHECK(alpha >= 0.0 && alpha <= 1.0, "mix_draw: ", name, " = ", alpha,
              " not in [0, 1]: the wave-wide Joehnk sampler needs alpha <= 1 "
              "(its acceptance rate falls below 1/2 above that)");
  return alpha > 0.0 ? (float)(1.0 / alpha) : 0.f;
}

inline unsigned long long unit_threshold(double p, const char* name) {
  TORCH_CHECK(p >= 0.0 && p <= 1.0, "mix_draw: ", name, " = ", p,
              " not in [0, 1]");
  return (unsigned long long)std::floor(p * 4294967296.0);
}

}  // namespace

int64_t mix_grid_cap() { return mix::kGridCap; }
int64_t mix_block() { return mix::kBlock; }

// Writes the record of (call_id, step scalar, key) for H x W images into
// `rec`.  `step` is the one-element int32 device scalar of ops/rng.py.
void mix_draw(torch::Tensor rec, torch::Tensor step, int64_t key0,
              int64_t key1, int64_t call_id, int64_t H, int64_t W,
              double alpha_mix, double alpha_cut, double prob,
              double switch_prob) {
  check_record(rec, "mix_draw");
  TORCH_CHECK(step.is_cuda() && step.numel() == 1 &&
                  step.scalar_type() == torch::kInt32 &&
                  step.device() == rec.device(),
              "mix_draw: step must be a one-element int32 tensor on the "
              "record's device");
  TORCH_CHECK(H >= 1 && W >= 1 && H * W < (1LL << 24),
              "mix_draw: H x W = ", H, " x ", W,
              " must be at least 1 x 1 and below 2^24 pixels (the box share "
              "is formed from exact fp32 integers)");
  mix::DrawArgs d;
  d.key0 = (uint32_t)key0;
  d.key1 = (uint32_t)key1;
  d.cid_lo = (uint32_t)((uint64_t)call_id & 0xffffffffu);
  d.cid_hi = (uint32_t)((uint64_t)call_id >> 32);
  d.thr_apply = unit_threshold(prob, "prob");
  d.thr_cut = unit_threshold(switch_prob, "switch_prob");
  d.H = (int)H;
  d.W = (int)W;
  d.inv_mix = inv_alpha(alpha_mix, "alpha_mix");
  d.inv_cut = inv_alpha(alpha_cut, "alpha_cut");
  TORCH_CHECK(d.inv_mix != 0.f || d.inv_cut != 0.f,
              "mix_draw: alpha_mix and alpha_cut are both 0");
  hipLaunchKernelGGL(mix::draw_kernel, dim3(1), dim3(kWave), 0,
                     c10::hip::getCurrentHIPStream(), rec.data_ptr<float>(),
                     reinterpret_cast<const uint32_t*>(step.data_ptr()), d);
}

// Mixes the contiguous image batch x [B, ...] in place under the record.
// xmul is C for NHWC and 1 for NCHW; the sample size must be a whole number
// of H x (W * xmul) planes.
torch::Tensor mix_batch_(torch::Tensor x, torch::Tensor rec, int64_t H,
                         int64_t W, int64_t xmul) {
  check_record(rec, "mix_batch_");
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.dim() >= 2 &&
                  x.device() == rec.device(),
              "mix_batch_: x must be a contiguous GPU batch on the record's "
              "device");
  const long long B = x.size(0);
  if (B < 2 || x.numel() == 0) return x;
  const long long n = x.numel() / B;
  const long long row = W * xmul;
  TORCH_CHECK(H >= 1 && W >= 1 && xmul >= 1 && n % (H * row) == 0,
              "mix_batch_: a sample of ", n, " elements is not a whole number "
              "of ", H, " x ", row, " planes");
  TORCH_CHECK(n < (1LL << 31) && B < (1LL << 31),
              "mix_batch_: sample size and batch must fit 31 bits");
  const long long pairs = (B + 1) / 2;
  DDP_DISPATCH_FLOAT(x.scalar_type(), "mix_batch_", [&] {
    constexpr int P = VecIO<scalar_t>::kPerLane;
    // vector route: every sample starts on a 16-byte boundary
    const bool vec = n % P == 0 && mix_aligned16(x.data_ptr());
    mix::MixArgs m;
    m.n = n;
    m.per = (uint32_t)(vec ? n / P : n);
    m.work = pairs * (long long)m.per;
    m.B = (uint32_t)B;
    m.row = (uint32_t)row;
    m.H = (uint32_t)H;
    m.xmul = (uint32_t)xmul;
    const int blocks = grid_1d(m.work, mix::kBlock, mix::kGridCap);
    auto stream = c10::hip::getCurrentHIPStream();
    auto* xp = reinterpret_cast<scalar_t*>(x.data_ptr());
    const float* rp = rec.data_ptr<float>();
    if (vec)
      hipLaunchKernelGGL((mix::batch_kernel<scalar_t, true>), dim3(blocks),
                         dim3(mix::kBlock), 0, stream, xp, rp, m);
    else
      hipLaunchKernelGGL((mix::batch_kernel<scalar_t, false>), dim3(blocks),
                         dim3(mix::kBlock), 0, stream, xp, rp, m);
  });
  return x;
}
