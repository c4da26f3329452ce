// Fused Philox dropout / stochastic depth / residual add (CDNA4, gfx950).
//
//   out = (res or 0) + x * keep_elem(e) * s_elem * keep_row(e / inner) * s_row
//
// One kernel family in the shape of ew::unary_kernel / binary_kernel: VecIO<T>
// 16 B per lane, a capped grid with a grid-stride loop and a scalar tail.
// Each mask and the residual are compile-time options; arithmetic is fp32 with
// one rounding to T; a dropped element contributes exactly res (or +0).
//
// The generator is Philox4x32-10 and it is stateless: element e of a call
// draws word (e & 3) of the block whose counter is
//   (e >> 2, call_id & 0xffffffff, call_id >> 32, step)
// under the key (key0, key1).  For the row mask e is the row index.  `step`
// is read from ONE device scalar, so a captured launch draws a fresh mask on
// every replay (ops/rng.py ticks it), and the backward is this same kernel on
// dy with the same (call_id, p, step scalar): no mask is ever stored.  The
// element and the row mask of one launch carry call ids of their own, so the
// two draws never share a word.
//
// Keep rule: keep iff word >= floor(p * 2^32); scale = float32(1 / (1 - p)),
// both formed in double on the host.  The block index always comes from the
// GLOBAL element index (never from the loop trip or the lane), so the vector
// body, the tail and the all-scalar route taken for a pointer that is not
// 16-B aligned draw the same bits.

#include <torch/extension.h>

#include <cmath>
#include <cstdint>

#include "common.h"
#include "dispatch.h"

namespace dp {

constexpr int kBlock = 256;
constexpr int kGridCap = 2048;

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

// word (i & 3) without indexing a register array
DEV_INLINE uint32_t pick(const U4& v, unsigned i) {
  const uint32_t lo = (i & 1) ? v.w1 : v.w0;
  const uint32_t hi = (i & 1) ? v.w3 : v.w2;
  return (i & 2) ? hi : lo;
}

struct Params {
  long long n;      // elements
  long long nvec;   // 16-B vectors taken by the vector body (0: all scalar)
  long long inner;  // elements per row (row mask)
  uint32_t key0, key1;
  uint32_t cid_e_lo, cid_e_hi;  // call id of the element mask
  uint32_t cid_r_lo, cid_r_hi;  // call id of the row mask
  uint32_t thr_e, thr_r;        // keep iff word >= thr
  float s_e, s_r;
};

DEV_INLINE unsigned long long udiv(unsigned long long a, unsigned long long b) {
  // rows and vectors fit 32 bits in every shape the models produce; the
  // 64-bit divide is the long way round
  if (((a | b) >> 32) == 0) return (uint32_t)a / (uint32_t)b;
  return a / b;
}

DEV_INLINE uint32_t draw(const Params& p, uint32_t cid_lo, uint32_t cid_hi,
                         unsigned long long e, uint32_t step) {
  return pick(philox((uint32_t)(e >> 2), cid_lo, cid_hi, step, p.key0, p.key1),
              (unsigned)(e & 3));
}

template <bool ELEM, bool ROW>
DEV_INLINE float scalar_term(const Params& p, long long e, float x,
                             uint32_t step) {
  float t = x;
  if (ELEM)
    t = draw(p, p.cid_e_lo, p.cid_e_hi, e, step) >= p.thr_e ? t * p.s_e : 0.f;
  if (ROW) {
    const unsigned long long row = udiv(e, p.inner);
    t = draw(p, p.cid_r_lo, p.cid_r_hi, row, step) >= p.thr_r ? t * p.s_r : 0.f;
  }
  return t;
}

template <typename T, bool ELEM, bool ROW, bool RES>
__global__ void dropout_kernel(const T* __restrict__ x,
                               const T* __restrict__ res, T* __restrict__ out,
                               const uint32_t* __restrict__ step_ptr,
                               Params p) {
  using IO = VecIO<T>;
  constexpr int P = IO::kPerLane;
  const uint32_t step = *step_ptr;
  const auto* vx = reinterpret_cast<const typename IO::Vec*>(x);
  const auto* vr = reinterpret_cast<const typename IO::Vec*>(res);
  auto* vo = reinterpret_cast<typename IO::Vec*>(out);
  const bool row_per_vec = ROW && (p.inner % P == 0);
  GRID_STRIDE(i, p.nvec) {
    typename IO::Vec v = vx[i], r, o;
    if (RES) r = vr[i];
    float t[P];
#pragma unroll
    for (int j = 0; j < P; ++j) t[j] = IO::get(v, j);
    if (ELEM) {
#pragma unroll
      for (int b = 0; b < P / 4; ++b) {
        const unsigned long long blk = (unsigned long long)i * (P / 4) + b;
        const U4 w = philox((uint32_t)blk, p.cid_e_lo, p.cid_e_hi, step,
                            p.key0, p.key1);
        t[4 * b + 0] = w.w0 >= p.thr_e ? t[4 * b + 0] * p.s_e : 0.f;
        t[4 * b + 1] = w.w1 >= p.thr_e ? t[4 * b + 1] * p.s_e : 0.f;
        t[4 * b + 2] = w.w2 >= p.thr_e ? t[4 * b + 2] * p.s_e : 0.f;
        t[4 * b + 3] = w.w3 >= p.thr_e ? t[4 * b + 3] * p.s_e : 0.f;
      }
    }
    if (ROW) {
      if (row_per_vec) {
        // the whole vector lies in one row: one draw
        const unsigned long long row =
            udiv((unsigned long long)i, (unsigned long long)(p.inner / P));
        const bool keep =
            draw(p, p.cid_r_lo, p.cid_r_hi, row, step) >= p.thr_r;
#pragma unroll
        for (int j = 0; j < P; ++j) t[j] = keep ? t[j] * p.s_r : 0.f;
      } else {
        unsigned long long row = udiv((unsigned long long)i * P, p.inner);
        long long left = (long long)(row + 1) * p.inner - i * P;  // in row
        bool keep = draw(p, p.cid_r_lo, p.cid_r_hi, row, step) >= p.thr_r;
#pragma unroll
        for (int j = 0; j < P; ++j) {
          if (left == 0) {
            ++row;
            left = p.inner;
            keep = draw(p, p.cid_r_lo, p.cid_r_hi, row, step) >= p.thr_r;
          }
          --left;
          t[j] = keep ? t[j] * p.s_r : 0.f;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < P; ++j)
      IO::set(o, j, RES ? IO::get(r, j) + t[j] : t[j]);
    vo[i] = o;
  }
  const long long base = p.nvec * P;
  GRID_STRIDE(i, p.n - base) {
    const long long e = base + i;
    const float t = scalar_term<ELEM, ROW>(p, e, to_f(x[e]), step);
    out[e] = to_t<T>(RES ? to_f(res[e]) + t : t);
  }
}

}  // namespace dp

// ======================= host launcher ===================================

namespace {

inline bool aligned16(const void* p) {
  return (reinterpret_cast<uintptr_t>(p) & 15u) == 0;
}

template <typename T, bool ELEM, bool ROW, bool RES>
void launch(const torch::Tensor& x, const torch::Tensor* res,
            torch::Tensor& out, const torch::Tensor& step, dp::Params p) {
  constexpr int P = VecIO<T>::kPerLane;
  const bool vec_ok = aligned16(x.data_ptr()) && aligned16(out.data_ptr()) &&
                      (!RES || aligned16(res->data_ptr()));
  p.nvec = vec_ok ? p.n / P : 0;
  const long long work = std::max(p.nvec, p.n - p.nvec * P);
  const int blocks = grid_1d(work, dp::kBlock, dp::kGridCap);
  hipLaunchKernelGGL(
      (dp::dropout_kernel<T, ELEM, ROW, RES>), dim3(blocks), dim3(dp::kBlock),
      0, c10::hip::getCurrentHIPStream(),
      reinterpret_cast<const T*>(x.data_ptr()),
      RES ? reinterpret_cast<const T*>(res->data_ptr()) : nullptr,
      reinterpret_cast<T*>(out.data_ptr()),
      reinterpret_cast<const uint32_t*>(step.data_ptr()), p);
}

template <typename T>
void route(bool elem, bool row, const torch::Tensor& x,
           const torch::Tensor* res, torch::Tensor& out,
           const torch::Tensor& step, const dp::Params& p) {
  const int sel = (elem ? 4 : 0) | (row ? 2 : 0) | (res ? 1 : 0);
  switch (sel) {
    case 2: return launch<T, false, true, false>(x, res, out, step, p);
    case 3: return launch<T, false, true, true>(x, res, out, step, p);
    case 4: return launch<T, true, false, false>(x, res, out, step, p);
    case 5: return launch<T, true, false, true>(x, res, out, step, p);
    case 6: return launch<T, true, true, false>(x, res, out, step, p);
    case 7: return launch<T, true, true, true>(x, res, out, step, p);
    default: TORCH_CHECK(false, "dropout_fwd: both rates are 0");
  }
}

inline uint32_t keep_threshold(double p) {
  TORCH_CHECK(p >= 0.0 && p < 1.0, "dropout_fwd: rate ", p, " not in [0, 1)");
  return (uint32_t)std::floor(p * 4294967296.0);
}

}  // namespace

int64_t dropout_grid_cap() { return dp::kGridCap; }
int64_t dropout_block() { return dp::kBlock; }

// x (and res, out) contiguous; `step` is the one-element int32 device scalar of
// ops/rng.py.  p_elem / p_row == 0 switches that mask off.  `inner` is the row
// length of the row mask.  Returns out (allocated here unless given).
torch::Tensor dropout_fwd(torch::Tensor x, c10::optional<torch::Tensor> res,
                          c10::optional<torch::Tensor> out_opt,
                          torch::Tensor step, int64_t key0, int64_t key1,
                          int64_t call_id_elem, int64_t call_id_row,
                          double p_elem, double p_row, int64_t inner) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous(),
              "dropout_fwd: x must be contiguous GPU");
  TORCH_CHECK(step.is_cuda() && step.numel() == 1 &&
                  step.scalar_type() == torch::kInt32 &&
                  step.device() == x.device(),
              "dropout_fwd: step must be a one-element int32 tensor on x's "
              "device");
  if (res.has_value())
    TORCH_CHECK(res->is_cuda() && res->is_contiguous() &&
                    res->scalar_type() == x.scalar_type() &&
                    res->numel() == x.numel() && res->device() == x.device(),
                "dropout_fwd: res must match x");
  torch::Tensor out = out_opt.has_value() ? *out_opt : torch::empty_like(x);
  TORCH_CHECK(out.is_cuda() && out.is_contiguous() &&
                  out.scalar_type() == x.scalar_type() &&
                  out.numel() == x.numel() && out.device() == x.device(),
              "dropout_fwd: out must match x");
  const long long n = x.numel();
  // the block index e >> 2 is one 32-bit counter word
  TORCH_CHECK(n < (1LL << 34), "dropout_fwd: more than 2^34 elements");
  const bool row = p_row > 0.0;
  if (row)
    TORCH_CHECK(inner >= 1 && n % inner == 0,
                "dropout_fwd: inner must divide numel");
  if (n == 0) return out;
  dp::Params p;
  p.n = n;
  p.nvec = 0;
  p.inner = row ? inner : 1;
  p.key0 = (uint32_t)key0;
  p.key1 = (uint32_t)key1;
  p.cid_e_lo = (uint32_t)((uint64_t)call_id_elem & 0xffffffffu);
  p.cid_e_hi = (uint32_t)((uint64_t)call_id_elem >> 32);
  p.cid_r_lo = (uint32_t)((uint64_t)call_id_row & 0xffffffffu);
  p.cid_r_hi = (uint32_t)((uint64_t)call_id_row >> 32);
  p.thr_e = keep_threshold(p_elem);
  p.thr_r = keep_threshold(p_row);
  p.s_e = (float)(1.0 / (1.0 - p_elem));
  p.s_r = (float)(1.0 / (1.0 - p_row));
  const torch::Tensor* rp = res.has_value() ? &*res : nullptr;
  DDP_DISPATCH_FLOAT(x.scalar_type(), "dropout_fwd", [&] {
    route<scalar_t>(p_elem > 0.0, row, x, rp, out, step, p);
  });
  return out;
}
