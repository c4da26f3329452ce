// Multi-tensor optimizer / gradient utilities (CDNA4, gfx950).
//
// Reference parity: SGD step (reference optim.SGD,
// ddp.py:183/240) as a fused multi-tensor kernel; global L2 grad norm +
// scale for clip_grad_norm_ (ddp.py:238-239).  Supports bf16 params with
// fp32 master weights (the apex-O2 slot, ddp.py:165-181, done natively).
// AdamW (the reference's apex FusedAdam slot) runs on the same
// machinery with its step count read from a device scalar.  LARS and LAMB
// add a per-tensor trust ratio to the two rules (norm / ratio / apply).
//
// Chunking: tensor lists are flattened into fixed-size chunks dispatched to
// blocks through a device-side descriptor table, so one launch covers the
// whole parameter set regardless of tensor count.

#include <torch/extension.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "common.h"
#include "dispatch.h"

namespace mt {

constexpr int kChunk = 1 << 13;  // elements per block chunk (8K: ResNet-18's
                                 // 11.7M params -> ~1.4K blocks, vs 64K chunks
                                 // which left the GPU <1 block/CU)
constexpr int kMaxTensors = 512;

struct ChunkDesc {
  int tensor;   // index into the pointer tables
  long long off;  // element offset of this chunk
};

struct PtrTable {
  const void* grad[kMaxTensors];
  void* param[kMaxTensors];
  float* mom[kMaxTensors];
  float* master[kMaxTensors];
  long long numel[kMaxTensors];
  float* aux[kMaxTensors];  // AdamW second moment (mom holds the first)
};

// ---- fused SGD (momentum / weight decay / dampening / nesterov) ----
// 4-wide aligned vector views (chunk offsets are kChunk-aligned and torch
// allocations are 256-B aligned, so only the final partial quad is scalar)
template <typename T>
struct alignas(8) Q4 {
  T v[4];
};
struct alignas(16) F4 {
  float v[4];
};

template <typename T>
__global__ void sgd_kernel(const ChunkDesc* __restrict__ chunks,
                           const PtrTable* __restrict__ tab, float lr,
                           float momentum, float wd, float damp, int nesterov,
                           int use_mom,
                           const float* __restrict__ guard = nullptr,
                           float* __restrict__ skip_count = nullptr,
                           const float* __restrict__ lr_dev = nullptr) {
  // lr can come from a device scalar so a hipGraph-captured step follows
  // the LIVE schedule (the host writes the new lr before each replay)
  if (lr_dev != nullptr) lr = *lr_dev;
  // Device-side skip: when the (pre-clip) grad norm is non-finite the whole
  // update is a no-op and a device counter ticks — the fp16 loss-scaler
  // reads that counter ONCE per sync interval instead of forcing a host
  // sync on every accumulation step.
  if (guard != nullptr && !isfinite(*guard)) {
    if (blockIdx.x == 0 && threadIdx.x == 0 && skip_count)
      atomicAdd(skip_count, 1.f);
    return;
  }
  const ChunkDesc d = chunks[blockIdx.x];
  const long long n = tab->numel[d.tensor];
  const long long base = d.off;
  const long long end = min(n, base + (long long)kChunk);
  const T* g = reinterpret_cast<const T*>(tab->grad[d.tensor]);
  T* p = reinterpret_cast<T*>(tab->param[d.tensor]);
  float* m = tab->mom[d.tensor];
  float* mw = tab->master[d.tensor];
  const long long vend = base + ((end - base) & ~3LL);
  for (long long i = base + (long long)threadIdx.x * 4; i < vend;
       i += (long long)blockDim.x * 4) {
    Q4<T> g4 = *reinterpret_cast<const Q4<T>*>(g + i);
    F4 w4, m4;
    if (mw) w4 = *reinterpret_cast<const F4*>(mw + i);
    Q4<T> p4;
    if (!mw) p4 = *reinterpret_cast<const Q4<T>*>(p + i);
    if (use_mom) m4 = *reinterpret_cast<const F4*>(m + i);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float gf = to_f(g4.v[j]);
      float w = mw ? w4.v[j] : to_f(p4.v[j]);
      if (wd != 0.f) gf += wd * w;
      if (use_mom) {
        float mv = m4.v[j] * momentum + (1.f - damp) * gf;
        m4.v[j] = mv;
        gf = nesterov ? gf + momentum * mv : mv;
      }
      w -= lr * gf;
      w4.v[j] = w;
      p4.v[j] = to_t<T>(w);
    }
    if (use_mom) *reinterpret_cast<F4*>(m + i) = m4;
    if (mw) *reinterpret_cast<F4*>(mw + i) = w4;
    *reinterpret_cast<Q4<T>*>(p + i) = p4;
  }
  for (long long i = vend + threadIdx.x; i < end; i += blockDim.x) {
    float gf = to_f(g[i]);
    float w = mw ? mw[i] : to_f(p[i]);
    if (wd != 0.f) gf += wd * w;
    if (use_mom) {
      float mv = m[i] * momentum + (1.f - damp) * gf;
      m[i] = mv;
      gf = nesterov ? gf + momentum * mv : mv;
    }
    w -= lr * gf;
    if (mw) mw[i] = w;
    p[i] = to_t<T>(w);
  }
}

// ---- fused AdamW (decoupled weight decay, torch.optim.AdamW rule) ----
// Per-launch constants, the same for every element.
struct AdamCoef {
  float lr_wd;      // lr * wd
  float b1, omb1;   // beta1, 1 - beta1 (1 - beta formed in double on the host)
  float b2, omb2;
  float step_size;  // lr / bc1
  float sqrt_bc2;
  float eps;
};

DEV_INLINE float adamw_update(float w, float g, float& m, float& v,
                              const AdamCoef& c) {
  w -= c.lr_wd * w;
  m = c.b1 * m + c.omb1 * g;
  v = c.b2 * v + c.omb2 * g * g;
  w -= c.step_size * m / (sqrtf(v) / c.sqrt_bc2 + c.eps);
  return w;
}

template <typename T>
__global__ void adamw_kernel(const ChunkDesc* __restrict__ chunks,
                             const PtrTable* __restrict__ tab, float lr,
                             float b1, float omb1, float log_b1, float b2,
                             float omb2, float log_b2, float eps, float wd,
                             const float* __restrict__ step,
                             const float* __restrict__ guard = nullptr,
                             const float* __restrict__ lr_dev = nullptr) {
  if (lr_dev != nullptr) lr = *lr_dev;
  // A skipped step is a no-op here; the optimizer advances neither the step
  // scalar nor the skip counter from this kernel (both tick once per step()
  // on the host side of the launch, however many plans a step needs).
  if (guard != nullptr && !isfinite(*guard)) return;
  // bias corrections 1 - beta^t from the LIVE device step count, through
  // expm1 of t * log(beta) (log taken in double on the host) so that small t
  // does not cancel; beta == 0 gives log = -inf and bc = 1.
  const float t = *step;
  AdamCoef c;
  c.lr_wd = lr * wd;
  c.b1 = b1;
  c.omb1 = omb1;
  c.b2 = b2;
  c.omb2 = omb2;
  c.step_size = lr / -expm1f(t * log_b1);
  c.sqrt_bc2 = sqrtf(-expm1f(t * log_b2));
  c.eps = eps;
  const ChunkDesc d = chunks[blockIdx.x];
  const long long n = tab->numel[d.tensor];
  const long long base = d.off;
  const long long end = min(n, base + (long long)kChunk);
  const T* g = reinterpret_cast<const T*>(tab->grad[d.tensor]);
  T* p = reinterpret_cast<T*>(tab->param[d.tensor]);
  float* m = tab->mom[d.tensor];
  float* v = tab->aux[d.tensor];
  float* mw = tab->master[d.tensor];
  const long long vend = base + ((end - base) & ~3LL);
  for (long long i = base + (long long)threadIdx.x * 4; i < vend;
       i += (long long)blockDim.x * 4) {
    Q4<T> g4 = *reinterpret_cast<const Q4<T>*>(g + i);
    F4 w4;
    if (mw) w4 = *reinterpret_cast<const F4*>(mw + i);
    Q4<T> p4;
    if (!mw) p4 = *reinterpret_cast<const Q4<T>*>(p + i);
    F4 m4 = *reinterpret_cast<const F4*>(m + i);
    F4 v4 = *reinterpret_cast<const F4*>(v + i);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float w = mw ? w4.v[j] : to_f(p4.v[j]);
      w = adamw_update(w, to_f(g4.v[j]), m4.v[j], v4.v[j], c);
      w4.v[j] = w;
      p4.v[j] = to_t<T>(w);
    }
    *reinterpret_cast<F4*>(m + i) = m4;
    *reinterpret_cast<F4*>(v + i) = v4;
    if (mw) *reinterpret_cast<F4*>(mw + i) = w4;
    *reinterpret_cast<Q4<T>*>(p + i) = p4;
  }
  for (long long i = vend + threadIdx.x; i < end; i += blockDim.x) {
    float mi = m[i], vi = v[i];
    float w = adamw_update(mw ? mw[i] : to_f(p[i]), to_f(g[i]), mi, vi, c);
    m[i] = mi;
    v[i] = vi;
    if (mw) mw[i] = w;
    p[i] = to_t<T>(w);
  }
}

// ---- sum of squares over a tensor list -> single f32 scalar ----
template <typename T>
__global__ void l2norm_sq_kernel(const ChunkDesc* __restrict__ chunks,
                                 const PtrTable* __restrict__ tab,
                                 float* __restrict__ out) {
  __shared__ float lds[4];
  const ChunkDesc d = chunks[blockIdx.x];
  const long long n = tab->numel[d.tensor];
  const long long base = d.off;
  const long long end = min(n, base + (long long)kChunk);
  const T* g = reinterpret_cast<const T*>(tab->grad[d.tensor]);
  float acc = 0.f;
  const long long vend = base + ((end - base) & ~3LL);
  for (long long i = base + (long long)threadIdx.x * 4; i < vend;
       i += (long long)blockDim.x * 4) {
    Q4<T> g4 = *reinterpret_cast<const Q4<T>*>(g + i);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float v = to_f(g4.v[j]);
      acc += v * v;
    }
  }
  for (long long i = vend + threadIdx.x; i < end; i += blockDim.x) {
    float v = to_f(g[i]);
    acc += v * v;
  }
  float total = block_reduce_sum<256>(acc, lds);
  if (threadIdx.x == 0) atomicAdd(out, total);
}

// ---- in-place scale by host scalar or device scalar ----
template <typename T>
__global__ void scale_kernel(const ChunkDesc* __restrict__ chunks,
                             const PtrTable* __restrict__ tab, float scale,
                             const float* __restrict__ dev_scale,
                             int clamp_to_one) {
  const ChunkDesc d = chunks[blockIdx.x];
  const long long n = tab->numel[d.tensor];
  const long long base = d.off;
  const long long end = min(n, base + (long long)kChunk);
  T* p = reinterpret_cast<T*>(tab->param[d.tensor]);
  float s = dev_scale ? *dev_scale : scale;
  if (clamp_to_one) s = fminf(s, 1.f);
  const long long vend = base + ((end - base) & ~3LL);
  for (long long i = base + (long long)threadIdx.x * 4; i < vend;
       i += (long long)blockDim.x * 4) {
    Q4<T> p4 = *reinterpret_cast<const Q4<T>*>(p + i);
#pragma unroll
    for (int j = 0; j < 4; ++j) p4.v[j] = to_t<T>(to_f(p4.v[j]) * s);
    *reinterpret_cast<Q4<T>*>(p + i) = p4;
  }
  for (long long i = vend + threadIdx.x; i < end; i += blockDim.x)
    p[i] = to_t<T>(to_f(p[i]) * s);
}

// ---- layer-wise trust ratios: LARS on SGD, LAMB on Adam ----
// A ratio needs one reduction per tensor that is complete before any element
// of the tensor moves, so each rule is three launches over the same plan:
//   norm   one block per chunk: the chunk's two sums of squares, reduced in a
//          fixed order and written to partial[chunk] with one plain store;
//   ratio  one wave per tensor: its partials in chunk order (a tensor's
//          chunks are contiguous in the chunk list) -> ratio[tensor];
//   apply  one block per chunk: the update, scaled by ratio[tensor].
// No atomics and no host: every sum has one order, so the ratios are the same
// bits on every run and on every rank that sees the same gradients.
struct LayerTable {
  int first_chunk[kMaxTensors];  // index of the tensor's first chunk
  int n_chunks[kMaxTensors];
  float wd[kMaxTensors];   // the tensor's weight decay
  int adapt[kMaxTensors];  // 0: ratio = 1
};

struct alignas(8) Sum2 {
  float a, b;
};

DEV_INLINE bool step_skipped(const float* __restrict__ guard) {
  return guard != nullptr && !isfinite(*guard);
}

// Both sums of a 256-thread block: the xor butterfly inside each wave, then
// the four wave sums left to right.  Valid in every thread.
DEV_INLINE Sum2 block_sum2(float a, float b, float* lds /*8*/) {
  a = wave_reduce_sum(a);
  b = wave_reduce_sum(b);
  if (lane_id() == 0) {
    lds[2 * wave_id()] = a;
    lds[2 * wave_id() + 1] = b;
  }
  __syncthreads();
  Sum2 s;
  s.a = ((lds[0] + lds[2]) + lds[4]) + lds[6];
  s.b = ((lds[1] + lds[3]) + lds[5]) + lds[7];
  return s;
}

// What every chunk kernel below needs from the tables.
template <typename T>
struct ChunkView {
  int tensor;
  long long base, vend, end;
  const T* g;
  T* p;
  float* m;
  float* v;
  float* mw;
  DEV_INLINE ChunkView(const ChunkDesc* __restrict__ chunks,
                       const PtrTable* __restrict__ tab) {
    const ChunkDesc d = chunks[blockIdx.x];
    tensor = d.tensor;
    base = d.off;
    end = min(tab->numel[d.tensor], base + (long long)kChunk);
    vend = base + ((end - base) & ~3LL);
    g = reinterpret_cast<const T*>(tab->grad[d.tensor]);
    p = reinterpret_cast<T*>(tab->param[d.tensor]);
    m = tab->mom[d.tensor];
    v = tab->aux[d.tensor];
    mw = tab->master[d.tensor];
  }
};

template <typename T>
__global__ void lars_norm_kernel(const ChunkDesc* __restrict__ chunks,
                                 const PtrTable* __restrict__ tab,
                                 const LayerTable* __restrict__ lay,
                                 Sum2* __restrict__ partial,
                                 const float* __restrict__ guard) {
  __shared__ float lds[8];
  if (step_skipped(guard)) return;
  const ChunkView<T> c(chunks, tab);
  // a tensor that does not adapt is not read: its ratio is 1 by the table
  if (!lay->adapt[c.tensor]) return;
  float gg = 0.f, ww = 0.f;
  for (long long i = c.base + (long long)threadIdx.x * 4; i < c.vend;
       i += (long long)blockDim.x * 4) {
    Q4<T> g4 = *reinterpret_cast<const Q4<T>*>(c.g + i);
    F4 w4;
    Q4<T> p4;
    if (c.mw) w4 = *reinterpret_cast<const F4*>(c.mw + i);
    if (!c.mw) p4 = *reinterpret_cast<const Q4<T>*>(c.p + i);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float gf = to_f(g4.v[j]);
      float w = c.mw ? w4.v[j] : to_f(p4.v[j]);
      gg += gf * gf;
      ww += w * w;
    }
  }
  for (long long i = c.vend + threadIdx.x; i < c.end; i += blockDim.x) {
    float gf = to_f(c.g[i]);
    float w = c.mw ? c.mw[i] : to_f(c.p[i]);
    gg += gf * gf;
    ww += w * w;
  }
  Sum2 s = block_sum2(gg, ww, lds);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// One wave per tensor, four tensors per block.  kLamb: partial = (|w|^2,
// |u|^2), ratio = |w| / |u|; else partial = (|g|^2, |w|^2) and
// ratio = eta * |w| / (|g| + wd * |w|).  Either is 1 where a norm is zero or
// the tensor does not adapt.
template <bool kLamb>
__global__ void layer_ratio_kernel(const LayerTable* __restrict__ lay,
                                   const Sum2* __restrict__ partial,
                                   float* __restrict__ ratio, int n_tensors,
                                   float eta,
                                   const float* __restrict__ guard) {
  if (step_skipped(guard)) return;
  const int t = blockIdx.x * (blockDim.x / kWave) + wave_id();
  if (t >= n_tensors) return;
  float r = 1.f;
  if (lay->adapt[t]) {
    const int first = lay->first_chunk[t];
    const int n = lay->n_chunks[t];
    float a = 0.f, b = 0.f;
    for (int k = lane_id(); k < n; k += kWave) {
      Sum2 s = partial[first + k];
      a += s.a;
      b += s.b;
    }
    a = sqrtf(wave_reduce_sum(a));
    b = sqrtf(wave_reduce_sum(b));
    if (a > 0.f && b > 0.f)
      r = kLamb ? a / b : eta * b / (a + lay->wd[t] * b);
  }
  if (lane_id() == 0) ratio[t] = r;
}

template <typename T>
__global__ void lars_apply_kernel(const ChunkDesc* __restrict__ chunks,
                                  const PtrTable* __restrict__ tab,
                                  const LayerTable* __restrict__ lay,
                                  const float* __restrict__ ratio, float lr,
                                  float momentum, float damp, int nesterov,
                                  int use_mom,
                                  const float* __restrict__ guard,
                                  const float* __restrict__ lr_dev) {
  if (lr_dev != nullptr) lr = *lr_dev;
  if (step_skipped(guard)) return;
  const ChunkView<T> c(chunks, tab);
  const float r = ratio[c.tensor];
  const float wd = lay->wd[c.tensor];
  const float omd = 1.f - damp;
  auto update = [&](float w, float gf, float& mv) {
    float d = r * (gf + wd * w);
    if (use_mom) {
      mv = momentum * mv + omd * d;
      d = nesterov ? d + momentum * mv : mv;
    }
    return w - lr * d;
  };
  for (long long i = c.base + (long long)threadIdx.x * 4; i < c.vend;
       i += (long long)blockDim.x * 4) {
    Q4<T> g4 = *reinterpret_cast<const Q4<T>*>(c.g + i);
    F4 w4, m4;
    Q4<T> p4;
    if (c.mw) w4 = *reinterpret_cast<const F4*>(c.mw + i);
    if (!c.mw) p4 = *reinterpret_cast<const Q4<T>*>(c.p + i);
    if (use_mom) m4 = *reinterpret_cast<const F4*>(c.m + i);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float w = update(c.mw ? w4.v[j] : to_f(p4.v[j]), to_f(g4.v[j]), m4.v[j]);
      w4.v[j] = w;
      p4.v[j] = to_t<T>(w);
    }
    if (use_mom) *reinterpret_cast<F4*>(c.m + i) = m4;
    if (c.mw) *reinterpret_cast<F4*>(c.mw + i) = w4;
    *reinterpret_cast<Q4<T>*>(c.p + i) = p4;
  }
  for (long long i = c.vend + threadIdx.x; i < c.end; i += blockDim.x) {
    float mv = use_mom ? c.m[i] : 0.f;
    float w = update(c.mw ? c.mw[i] : to_f(c.p[i]), to_f(c.g[i]), mv);
    if (use_mom) c.m[i] = mv;
    if (c.mw) c.mw[i] = w;
    c.p[i] = to_t<T>(w);
  }
}

// LAMB's per-launch constants; 1 - beta^t as in adamw_kernel.
struct LambCoef {
  float b1, omb1, b2, omb2;
  float inv_bc1;   // 1 / (1 - beta1^t)
  float sqrt_bc2;  // sqrt(1 - beta2^t)
  float eps;
  DEV_INLINE LambCoef(float b1_, float omb1_, float log_b1, float b2_,
                      float omb2_, float log_b2, float eps_, float t)
      : b1(b1_), omb1(omb1_), b2(b2_), omb2(omb2_),
        inv_bc1(1.f / -expm1f(t * log_b1)),
        sqrt_bc2(sqrtf(-expm1f(t * log_b2))), eps(eps_) {}
};

// u = m_hat / (sqrt(v_hat) + eps) + wd * w.  The norm pass and the apply pass
// both form it here from the stored m and v: storing u instead would move as
// many bytes and cost an fp32 buffer the size of the parameters.
DEV_INLINE float lamb_u(float m, float v, float w, float wd,
                        const LambCoef& c) {
  return (m * c.inv_bc1) / (sqrtf(v) / c.sqrt_bc2 + c.eps) + wd * w;
}

template <typename T>
__global__ void lamb_norm_kernel(const ChunkDesc* __restrict__ chunks,
                                 const PtrTable* __restrict__ tab,
                                 const LayerTable* __restrict__ lay,
                                 Sum2* __restrict__ partial, float b1,
                                 float omb1, float log_b1, float b2,
                                 float omb2, float log_b2, float eps,
                                 const float* __restrict__ step,
                                 const float* __restrict__ guard) {
  __shared__ float lds[8];
  if (step_skipped(guard)) return;
  const LambCoef k(b1, omb1, log_b1, b2, omb2, log_b2, eps, *step);
  const ChunkView<T> c(chunks, tab);
  const float wd = lay->wd[c.tensor];
  float ww = 0.f, uu = 0.f;
  auto moments = [&](float w, float gf, float& m, float& v) {
    m = k.b1 * m + k.omb1 * gf;
    v = k.b2 * v + k.omb2 * gf * gf;
    float u = lamb_u(m, v, w, wd, k);
    ww += w * w;
    uu += u * u;
  };
  for (long long i = c.base + (long long)threadIdx.x * 4; i < c.vend;
       i += (long long)blockDim.x * 4) {
    Q4<T> g4 = *reinterpret_cast<const Q4<T>*>(c.g + i);
    F4 w4;
    Q4<T> p4;
    if (c.mw) w4 = *reinterpret_cast<const F4*>(c.mw + i);
    if (!c.mw) p4 = *reinterpret_cast<const Q4<T>*>(c.p + i);
    F4 m4 = *reinterpret_cast<const F4*>(c.m + i);
    F4 v4 = *reinterpret_cast<const F4*>(c.v + i);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      moments(c.mw ? w4.v[j] : to_f(p4.v[j]), to_f(g4.v[j]), m4.v[j],
              v4.v[j]);
    *reinterpret_cast<F4*>(c.m + i) = m4;
    *reinterpret_cast<F4*>(c.v + i) = v4;
  }
  for (long long i = c.vend + threadIdx.x; i < c.end; i += blockDim.x) {
    float mi = c.m[i], vi = c.v[i];
    moments(c.mw ? c.mw[i] : to_f(c.p[i]), to_f(c.g[i]), mi, vi);
    c.m[i] = mi;
    c.v[i] = vi;
  }
  // the moments move whether or not the tensor adapts; its sums are read
  // only if it does
  if (!lay->adapt[c.tensor]) return;
  Sum2 s = block_sum2(ww, uu, lds);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

template <typename T>
__global__ void lamb_apply_kernel(const ChunkDesc* __restrict__ chunks,
                                  const PtrTable* __restrict__ tab,
                                  const LayerTable* __restrict__ lay,
                                  const float* __restrict__ ratio, float lr,
                                  float b1, float omb1, float log_b1,
                                  float b2, float omb2, float log_b2,
                                  float eps, const float* __restrict__ step,
                                  const float* __restrict__ guard,
                                  const float* __restrict__ lr_dev) {
  if (lr_dev != nullptr) lr = *lr_dev;
  if (step_skipped(guard)) return;
  const LambCoef k(b1, omb1, log_b1, b2, omb2, log_b2, eps, *step);
  const ChunkView<T> c(chunks, tab);
  const float wd = lay->wd[c.tensor];
  const float lr_r = lr * ratio[c.tensor];
  for (long long i = c.base + (long long)threadIdx.x * 4; i < c.vend;
       i += (long long)blockDim.x * 4) {
    F4 w4;
    Q4<T> p4;
    if (c.mw) w4 = *reinterpret_cast<const F4*>(c.mw + i);
    if (!c.mw) p4 = *reinterpret_cast<const Q4<T>*>(c.p + i);
    F4 m4 = *reinterpret_cast<const F4*>(c.m + i);
    F4 v4 = *reinterpret_cast<const F4*>(c.v + i);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float w = c.mw ? w4.v[j] : to_f(p4.v[j]);
      w -= lr_r * lamb_u(m4.v[j], v4.v[j], w, wd, k);
      w4.v[j] = w;
      p4.v[j] = to_t<T>(w);
    }
    if (c.mw) *reinterpret_cast<F4*>(c.mw + i) = w4;
    *reinterpret_cast<Q4<T>*>(c.p + i) = p4;
  }
  for (long long i = c.vend + threadIdx.x; i < c.end; i += blockDim.x) {
    float w = c.mw ? c.mw[i] : to_f(c.p[i]);
    w -= lr_r * lamb_u(c.m[i], c.v[i], w, wd, k);
    if (c.mw) c.mw[i] = w;
    c.p[i] = to_t<T>(w);
  }
}

}  // namespace mt

// ======================= host side =======================================

namespace {

struct LaunchPlan {
  torch::Tensor chunks_dev;   // ChunkDesc[]
  torch::Tensor table_dev;    // PtrTable
  torch::Tensor chunks_host;  // PINNED sources kept alive: a hipGraph-
  torch::Tensor table_host;   // captured H2D copy replays from this memory
  int n_blocks;
  int n_tensors;
  // layer-wise steps only (add_layer_state): they live as long as the
  // tables, so a captured step replays against the same pointers
  torch::Tensor layer_dev;   // LayerTable
  torch::Tensor layer_host;  // its pinned source
  torch::Tensor partial;     // Sum2[n_blocks]
  torch::Tensor ratio;       // float[n_tensors], created as ones
  bool adapt = false;        // false: ratio is never written and stays 1
};

// Plan cache: the descriptor tables depend only on the tensor PTRS/numels,
// which are stable across steps when grads are zeroed in place (and must be
// stable under hipGraph capture).  Caching (a) keeps the HOST staging
// tensors alive so a captured H2D copy replays from live memory, and
// (b) removes the per-step host build + H2D copy on the hot path.
struct PlanKey {
  std::vector<const void*> ptrs;
  bool operator==(const PlanKey& o) const { return ptrs == o.ptrs; }
};
struct PlanEntry {
  PlanKey key;
  std::vector<LaunchPlan> plans;
};

std::vector<PlanEntry>& plan_cache() {
  static std::vector<PlanEntry> c;
  return c;
}

template <typename Build>
const std::vector<LaunchPlan>& cached_plans(PlanKey&& key, Build build) {
  auto& cache = plan_cache();
  for (auto& e : cache)
    if (e.key == key) return e.plans;
  if (cache.size() >= 64) cache.clear();  // bound (param sets rarely churn)
  cache.push_back(PlanEntry{std::move(key), build()});
  return cache.back().plans;
}

// Build chunk descriptors + pointer table on host, copy to device once per
// call (tiny: ~KBs).  Lists longer than kMaxTensors are processed in groups.
template <typename FillPtrs>
std::vector<LaunchPlan> make_plans(const std::vector<torch::Tensor>& ref,
                                   const torch::Device& dev, FillPtrs fill) {
  std::vector<LaunchPlan> plans;
  size_t t = 0;
  while (t < ref.size()) {
    size_t t_end = std::min(ref.size(), t + (size_t)mt::kMaxTensors);
    auto table_host = torch::empty(
        {(long long)sizeof(mt::PtrTable)},
        torch::dtype(torch::kUInt8).pinned_memory(true));
    auto* tab = reinterpret_cast<mt::PtrTable*>(table_host.data_ptr());
    std::vector<mt::ChunkDesc> chunks;
    for (size_t i = t; i < t_end; ++i) {
      int local = (int)(i - t);
      fill(i, local, tab);
      long long n = ref[i].numel();
      tab->numel[local] = n;
      for (long long off = 0; off < n; off += mt::kChunk)
        chunks.push_back({local, off});
    }
    LaunchPlan plan;
    plan.chunks_host = torch::from_blob(
                           chunks.data(),
                           {(long long)(chunks.size() * sizeof(mt::ChunkDesc))},
                           torch::dtype(torch::kUInt8))
                           .pin_memory();
    plan.table_host = table_host;
    plan.chunks_dev = plan.chunks_host.to(dev, /*non_blocking=*/true);
    plan.table_dev = plan.table_host.to(dev, /*non_blocking=*/true);
    plan.n_blocks = (int)chunks.size();
    plan.n_tensors = (int)(t_end - t);
    plans.push_back(plan);
    t = t_end;
  }
  return plans;
}

// Give each plan what a layer-wise step needs on top of the tables: where
// each tensor's chunks lie in the chunk list (read back from the list
// itself), its weight decay and whether it adapts, and the buffers for the
// chunk sums and the ratios.  A tensor never spans plans, so neither does
// its norm.
std::vector<LaunchPlan> add_layer_state(std::vector<LaunchPlan> plans,
                                        const torch::Device& dev, float wd,
                                        bool adapt) {
  for (auto& plan : plans) {
    plan.layer_host = torch::empty(
        {(long long)sizeof(mt::LayerTable)},
        torch::dtype(torch::kUInt8).pinned_memory(true));
    auto* lay = reinterpret_cast<mt::LayerTable*>(plan.layer_host.data_ptr());
    for (int i = 0; i < mt::kMaxTensors; ++i) {
      lay->first_chunk[i] = 0;
      lay->n_chunks[i] = 0;
      lay->wd[i] = wd;
      lay->adapt[i] = adapt ? 1 : 0;
    }
    auto* chunks =
        reinterpret_cast<const mt::ChunkDesc*>(plan.chunks_host.data_ptr());
    for (int k = 0; k < plan.n_blocks; ++k) {
      const int tensor = chunks[k].tensor;
      TORCH_CHECK(tensor >= 0 && tensor < plan.n_tensors);
      if (lay->n_chunks[tensor]++ == 0) lay->first_chunk[tensor] = k;
      TORCH_CHECK(lay->first_chunk[tensor] + lay->n_chunks[tensor] == k + 1,
                  "a tensor's chunks must be contiguous in the chunk list");
    }
    plan.layer_dev = plan.layer_host.to(dev, /*non_blocking=*/true);
    auto f32 = torch::dtype(torch::kFloat32).device(dev);
    plan.partial = torch::zeros({std::max(plan.n_blocks, 1), 2}, f32);
    plan.ratio = torch::ones({plan.n_tensors}, f32);
    plan.adapt = adapt;
  }
  return plans;
}

// The three launches of one layer-wise step over one plan; norm and apply
// are given the plan's pointers and launch their kernel.  A plan whose group
// does not adapt keeps the ones its ratios were created with: it skips the
// ratio launch, and LARS, whose norm pass writes nothing else, that one too.
template <bool kLamb, typename Norm, typename Apply>
void launch_layer_step(const LaunchPlan& plan, hipStream_t stream, float eta,
                       const float* guard, Norm norm, Apply apply) {
  if (plan.n_blocks == 0) return;
  auto* chunks =
      reinterpret_cast<const mt::ChunkDesc*>(plan.chunks_dev.data_ptr());
  auto* tab = reinterpret_cast<const mt::PtrTable*>(plan.table_dev.data_ptr());
  auto* lay =
      reinterpret_cast<const mt::LayerTable*>(plan.layer_dev.data_ptr());
  auto* partial = reinterpret_cast<mt::Sum2*>(plan.partial.data_ptr());
  float* ratio = plan.ratio.data_ptr<float>();
  if (kLamb || plan.adapt) norm(chunks, tab, lay, partial);
  if (plan.adapt)
    hipLaunchKernelGGL((mt::layer_ratio_kernel<kLamb>),
                       dim3((plan.n_tensors + 3) / 4), dim3(256), 0, stream,
                       lay, partial, ratio, plan.n_tensors, eta, guard);
  apply(chunks, tab, lay, ratio);
}

}  // namespace

void sgd_step(std::vector<torch::Tensor> params, std::vector<torch::Tensor> grads,
              std::vector<torch::Tensor> moms, std::vector<torch::Tensor> masters,
              double lr, double momentum, double wd, double damp,
              bool nesterov, c10::optional<torch::Tensor> guard,
              c10::optional<torch::Tensor> skip_count,
              c10::optional<torch::Tensor> lr_tensor) {
  TORCH_CHECK(!params.empty());
  auto dev = params[0].device();
  const float* guard_p = nullptr;
  float* skip_p = nullptr;
  if (guard.has_value()) {
    TORCH_CHECK(guard->scalar_type() == torch::kFloat32 && guard->numel() == 1);
    guard_p = guard->data_ptr<float>();
  }
  if (skip_count.has_value()) {
    TORCH_CHECK(skip_count->scalar_type() == torch::kFloat32 &&
                skip_count->numel() == 1);
    skip_p = skip_count->data_ptr<float>();
  }
  const float* lr_p = nullptr;
  if (lr_tensor.has_value()) {
    TORCH_CHECK(lr_tensor->scalar_type() == torch::kFloat32 &&
                lr_tensor->numel() == 1);
    lr_p = lr_tensor->data_ptr<float>();
  }
  const bool use_mom = momentum != 0.0;
  PlanKey key;
  key.ptrs.reserve(4 * params.size() + 2);
  key.ptrs.push_back((const void*)0x56D);  // op tag
  key.ptrs.push_back((const void*)(uintptr_t)params.size());
  for (size_t i = 0; i < params.size(); ++i) {
    key.ptrs.push_back(params[i].data_ptr());
    key.ptrs.push_back(grads[i].data_ptr());
    key.ptrs.push_back((const void*)(uintptr_t)params[i].numel());
    key.ptrs.push_back(
        (use_mom && moms[i].defined() && moms[i].numel()) ? moms[i].data_ptr()
                                                          : nullptr);
    key.ptrs.push_back((masters[i].defined() && masters[i].numel())
                           ? masters[i].data_ptr()
                           : nullptr);
  }
  const auto& plans = cached_plans(std::move(key), [&] {
    return make_plans(
        params, dev, [&](size_t i, int local, mt::PtrTable* tab) {
          tab->grad[local] = grads[i].data_ptr();
          tab->param[local] = params[i].data_ptr();
          tab->mom[local] =
              (use_mom && moms[i].defined() && moms[i].numel())
                  ? moms[i].data_ptr<float>()
                  : nullptr;
          tab->master[local] =
              (masters[i].defined() && masters[i].numel())
                  ? masters[i].data_ptr<float>()
                  : nullptr;
        });
  });
  auto stream = c10::hip::getCurrentHIPStream();
  for (auto& plan : plans) {
    DDP_DISPATCH_FLOAT(params[0].scalar_type(), "sgd_step", [&] {
      hipLaunchKernelGGL(
          (mt::sgd_kernel<scalar_t>), dim3(plan.n_blocks), dim3(256), 0,
          stream,
          reinterpret_cast<const mt::ChunkDesc*>(plan.chunks_dev.data_ptr()),
          reinterpret_cast<const mt::PtrTable*>(plan.table_dev.data_ptr()),
          (float)lr, (float)momentum, (float)wd, (float)damp, nesterov ? 1 : 0,
          use_mom ? 1 : 0, guard_p, skip_p, lr_p);
    });
  }
}

// AdamW over a tensor list.  `step` is the optimizer's device step count
// (already advanced for this step by the caller); see optim.AdamW.
void adamw_step(std::vector<torch::Tensor> params,
                std::vector<torch::Tensor> grads,
                std::vector<torch::Tensor> exp_avgs,
                std::vector<torch::Tensor> exp_avg_sqs,
                std::vector<torch::Tensor> masters, double lr, double beta1,
                double beta2, double eps, double wd, torch::Tensor step,
                c10::optional<torch::Tensor> guard,
                c10::optional<torch::Tensor> skip_count,
                c10::optional<torch::Tensor> lr_tensor) {
  TORCH_CHECK(!params.empty(), "adamw_step: empty parameter list");
  const size_t n = params.size();
  TORCH_CHECK(grads.size() == n && exp_avgs.size() == n &&
                  exp_avg_sqs.size() == n && masters.size() == n,
              "adamw_step: list lengths differ");
  TORCH_CHECK(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0,
              "adamw_step: betas must be in [0, 1)");
  auto dev = params[0].device();
  const auto dtype = params[0].scalar_type();
  auto f32_scalar = [&](const torch::Tensor& t, const char* what) {
    TORCH_CHECK(t.scalar_type() == torch::kFloat32 && t.numel() == 1 &&
                    t.device() == dev,
                "adamw_step: ", what,
                " must be a one-element f32 tensor on the params' device");
    return t.data_ptr<float>();
  };
  auto f32_state = [&](const torch::Tensor& t, size_t i, const char* what) {
    TORCH_CHECK(t.scalar_type() == torch::kFloat32 && t.is_contiguous() &&
                    t.numel() == params[i].numel() && t.device() == dev,
                "adamw_step: ", what, "[", i,
                "] must be contiguous f32 with the param's numel");
    return t.data_ptr<float>();
  };
  const float* step_p = f32_scalar(step, "step");
  const float* guard_p =
      guard.has_value() ? f32_scalar(*guard, "guard") : nullptr;
  // the skip counter is ticked by the caller once per step, never here
  if (skip_count.has_value()) f32_scalar(*skip_count, "skip_count");
  const float* lr_p =
      lr_tensor.has_value() ? f32_scalar(*lr_tensor, "lr_tensor") : nullptr;
  std::vector<float*> m_p(n), v_p(n), mw_p(n);
  for (size_t i = 0; i < n; ++i) {
    TORCH_CHECK(params[i].scalar_type() == dtype &&
                    grads[i].scalar_type() == dtype,
                "adamw_step: param/grad ", i, " dtype differs from params[0]");
    TORCH_CHECK(params[i].is_contiguous() && grads[i].is_contiguous(),
                "adamw_step: param/grad ", i, " is not contiguous");
    TORCH_CHECK(grads[i].numel() == params[i].numel() &&
                    params[i].device() == dev && grads[i].device() == dev,
                "adamw_step: param/grad ", i, " numel or device mismatch");
    m_p[i] = f32_state(exp_avgs[i], i, "exp_avgs");
    v_p[i] = f32_state(exp_avg_sqs[i], i, "exp_avg_sqs");
    mw_p[i] = (masters[i].defined() && masters[i].numel())
                  ? f32_state(masters[i], i, "masters")
                  : nullptr;
  }
  PlanKey key;
  key.ptrs.reserve(6 * n + 2);
  key.ptrs.push_back((const void*)0xADA3);  // op tag
  key.ptrs.push_back((const void*)(uintptr_t)n);
  for (size_t i = 0; i < n; ++i) {
    key.ptrs.push_back(params[i].data_ptr());
    key.ptrs.push_back(grads[i].data_ptr());
    key.ptrs.push_back((const void*)(uintptr_t)params[i].numel());
    key.ptrs.push_back(m_p[i]);
    key.ptrs.push_back(v_p[i]);
    key.ptrs.push_back(mw_p[i]);
  }
  const auto& plans = cached_plans(std::move(key), [&] {
    return make_plans(params, dev,
                      [&](size_t i, int local, mt::PtrTable* tab) {
                        tab->grad[local] = grads[i].data_ptr();
                        tab->param[local] = params[i].data_ptr();
                        tab->mom[local] = m_p[i];
                        tab->aux[local] = v_p[i];
                        tab->master[local] = mw_p[i];
                      });
  });
  // log(beta) in double: the kernel forms 1 - beta^t as -expm1(t * log beta)
  const float log_b1 = (float)std::log(beta1);
  const float log_b2 = (float)std::log(beta2);
  auto stream = c10::hip::getCurrentHIPStream();
  for (auto& plan : plans) {
    DDP_DISPATCH_FLOAT(dtype, "adamw_step", [&] {
      hipLaunchKernelGGL(
          (mt::adamw_kernel<scalar_t>), dim3(plan.n_blocks), dim3(256), 0,
          stream,
          reinterpret_cast<const mt::ChunkDesc*>(plan.chunks_dev.data_ptr()),
          reinterpret_cast<const mt::PtrTable*>(plan.table_dev.data_ptr()),
          (float)lr, (float)beta1, (float)(1.0 - beta1), log_b1, (float)beta2,
          (float)(1.0 - beta2), log_b2, (float)eps, (float)wd, step_p, guard_p,
          lr_p);
    });
  }
}

// ---- layer-wise steps: LARS (optim.SGD, trust_coef > 0) and LAMB
// (optim.AdamW, trust_ratio=True).  One call is one param group of one dtype:
// lr, momentum / betas and eps are the group's, and so are wd and adapt,
// which travel per tensor in the plan's LayerTable and are part of its key.
// Neither ticks skip_count: the optimizers do that once per step().
namespace {

struct LayerArgs {
  torch::Device dev;
  torch::ScalarType dtype;
  const float* guard = nullptr;
  const float* lr = nullptr;
  std::vector<float*> master;

  // checks shared by both steps; f32_state checks one state list
  LayerArgs(const char* op, const std::vector<torch::Tensor>& params,
            const std::vector<torch::Tensor>& grads,
            const std::vector<torch::Tensor>& masters,
            const c10::optional<torch::Tensor>& guard_t,
            const c10::optional<torch::Tensor>& lr_t)
      : dev(torch::kCPU), dtype(torch::kFloat32), op_(op) {
    TORCH_CHECK(!params.empty(), op_, ": empty parameter list");
    TORCH_CHECK(grads.size() == params.size() &&
                    masters.size() == params.size(),
                op_, ": list lengths differ");
    dev = params[0].device();
    dtype = params[0].scalar_type();
    if (guard_t.has_value()) guard = scalar(*guard_t, "guard");
    if (lr_t.has_value()) lr = scalar(*lr_t, "lr_tensor");
    for (size_t i = 0; i < params.size(); ++i) {
      TORCH_CHECK(params[i].scalar_type() == dtype &&
                      grads[i].scalar_type() == dtype,
                  op_, ": param/grad ", i, " dtype differs from params[0]");
      TORCH_CHECK(params[i].is_contiguous() && grads[i].is_contiguous() &&
                      grads[i].numel() == params[i].numel() &&
                      params[i].device() == dev && grads[i].device() == dev,
                  op_, ": param/grad ", i,
                  " must be contiguous, of one numel, on params[0]'s device");
    }
    master = f32_state(params, masters, "masters", /*optional=*/true);
  }

  const float* scalar(const torch::Tensor& t, const char* what) const {
    TORCH_CHECK(t.scalar_type() == torch::kFloat32 && t.numel() == 1 &&
                    t.device() == dev,
                op_, ": ", what,
                " must be a one-element f32 tensor on the params' device");
    return t.data_ptr<float>();
  }

  std::vector<float*> f32_state(const std::vector<torch::Tensor>& params,
                                const std::vector<torch::Tensor>& ts,
                                const char* what, bool optional) const {
    TORCH_CHECK(ts.size() == params.size(), op_, ": list lengths differ");
    std::vector<float*> out(ts.size(), nullptr);
    for (size_t i = 0; i < ts.size(); ++i) {
      if (optional && !(ts[i].defined() && ts[i].numel())) continue;
      TORCH_CHECK(ts[i].scalar_type() == torch::kFloat32 &&
                      ts[i].is_contiguous() &&
                      ts[i].numel() == params[i].numel() &&
                      ts[i].device() == dev,
                  op_, ": ", what, "[", i,
                  "] must be contiguous f32 with the param's numel");
      out[i] = ts[i].data_ptr<float>();
    }
    return out;
  }

 private:
  const char* op_;
};

const void* float_bits(float v) {
  uint32_t u;
  std::memcpy(&u, &v, sizeof u);
  return (const void*)(uintptr_t)u;
}

}  // namespace

void lars_step(std::vector<torch::Tensor> params,
               std::vector<torch::Tensor> grads,
               std::vector<torch::Tensor> moms,
               std::vector<torch::Tensor> masters, double lr, double momentum,
               double wd, double damp, bool nesterov, double trust_coef,
               bool adapt, c10::optional<torch::Tensor> guard,
               c10::optional<torch::Tensor> lr_tensor) {
  const LayerArgs a("lars_step", params, grads, masters, guard, lr_tensor);
  TORCH_CHECK(trust_coef > 0.0 || !adapt,
              "lars_step: a group that adapts needs trust_coef > 0");
  const bool use_mom = momentum != 0.0;
  const auto m_p = a.f32_state(params, moms, "moms", /*optional=*/!use_mom);
  const size_t n = params.size();
  PlanKey key;
  key.ptrs.reserve(5 * n + 4);
  key.ptrs.push_back((const void*)0x1A25);  // op tag
  key.ptrs.push_back((const void*)(uintptr_t)n);
  key.ptrs.push_back(float_bits((float)wd));
  key.ptrs.push_back((const void*)(uintptr_t)adapt);
  for (size_t i = 0; i < n; ++i) {
    key.ptrs.push_back(params[i].data_ptr());
    key.ptrs.push_back(grads[i].data_ptr());
    key.ptrs.push_back((const void*)(uintptr_t)params[i].numel());
    key.ptrs.push_back(use_mom ? m_p[i] : nullptr);
    key.ptrs.push_back(a.master[i]);
  }
  const auto& plans = cached_plans(std::move(key), [&] {
    return add_layer_state(
        make_plans(params, a.dev,
                   [&](size_t i, int local, mt::PtrTable* tab) {
                     tab->grad[local] = grads[i].data_ptr();
                     tab->param[local] = params[i].data_ptr();
                     tab->mom[local] = use_mom ? m_p[i] : nullptr;
                     tab->aux[local] = nullptr;
                     tab->master[local] = a.master[i];
                   }),
        a.dev, (float)wd, adapt);
  });
  auto stream = c10::hip::getCurrentHIPStream();
  for (auto& plan : plans) {
    DDP_DISPATCH_FLOAT(a.dtype, "lars_step", [&] {
      launch_layer_step</*kLamb=*/false>(
          plan, stream, (float)trust_coef, a.guard,
          [&](auto chunks, auto tab, auto lay, auto partial) {
            hipLaunchKernelGGL((mt::lars_norm_kernel<scalar_t>),
                               dim3(plan.n_blocks), dim3(256), 0, stream,
                               chunks, tab, lay, partial, a.guard);
          },
          [&](auto chunks, auto tab, auto lay, auto ratio) {
            hipLaunchKernelGGL((mt::lars_apply_kernel<scalar_t>),
                               dim3(plan.n_blocks), dim3(256), 0, stream,
                               chunks, tab, lay, ratio, (float)lr,
                               (float)momentum, (float)damp, nesterov ? 1 : 0,
                               use_mom ? 1 : 0, a.guard, a.lr);
          });
    });
  }
}

// `step` is the optimizer's device step count, already advanced for this
// step by the caller, as for adamw_step.
void lamb_step(std::vector<torch::Tensor> params,
               std::vector<torch::Tensor> grads,
               std::vector<torch::Tensor> exp_avgs,
               std::vector<torch::Tensor> exp_avg_sqs,
               std::vector<torch::Tensor> masters, double lr, double beta1,
               double beta2, double eps, double wd, bool adapt,
               torch::Tensor step, c10::optional<torch::Tensor> guard,
               c10::optional<torch::Tensor> lr_tensor) {
  const LayerArgs a("lamb_step", params, grads, masters, guard, lr_tensor);
  TORCH_CHECK(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0,
              "lamb_step: betas must be in [0, 1)");
  const float* step_p = a.scalar(step, "step");
  const auto m_p = a.f32_state(params, exp_avgs, "exp_avgs", false);
  const auto v_p = a.f32_state(params, exp_avg_sqs, "exp_avg_sqs", false);
  const size_t n = params.size();
  PlanKey key;
  key.ptrs.reserve(6 * n + 4);
  key.ptrs.push_back((const void*)0x1A3B);  // op tag
  key.ptrs.push_back((const void*)(uintptr_t)n);
  key.ptrs.push_back(float_bits((float)wd));
  key.ptrs.push_back((const void*)(uintptr_t)adapt);
  for (size_t i = 0; i < n; ++i) {
    key.ptrs.push_back(params[i].data_ptr());
    key.ptrs.push_back(grads[i].data_ptr());
    key.ptrs.push_back((const void*)(uintptr_t)params[i].numel());
    key.ptrs.push_back(m_p[i]);
    key.ptrs.push_back(v_p[i]);
    key.ptrs.push_back(a.master[i]);
  }
  const auto& plans = cached_plans(std::move(key), [&] {
    return add_layer_state(
        make_plans(params, a.dev,
                   [&](size_t i, int local, mt::PtrTable* tab) {
                     tab->grad[local] = grads[i].data_ptr();
                     tab->param[local] = params[i].data_ptr();
                     tab->mom[local] = m_p[i];
                     tab->aux[local] = v_p[i];
                     tab->master[local] = a.master[i];
                   }),
        a.dev, (float)wd, adapt);
  });
  const float b1 = (float)beta1, omb1 = (float)(1.0 - beta1);
  const float b2 = (float)beta2, omb2 = (float)(1.0 - beta2);
  const float log_b1 = (float)std::log(beta1);
  const float log_b2 = (float)std::log(beta2);
  auto stream = c10::hip::getCurrentHIPStream();
  for (auto& plan : plans) {
    DDP_DISPATCH_FLOAT(a.dtype, "lamb_step", [&] {
      launch_layer_step</*kLamb=*/true>(
          plan, stream, 0.f, a.guard,
          [&](auto chunks, auto tab, auto lay, auto partial) {
            hipLaunchKernelGGL((mt::lamb_norm_kernel<scalar_t>),
                               dim3(plan.n_blocks), dim3(256), 0, stream,
                               chunks, tab, lay, partial, b1, omb1, log_b1,
                               b2, omb2, log_b2, (float)eps, step_p, a.guard);
          },
          [&](auto chunks, auto tab, auto lay, auto ratio) {
            hipLaunchKernelGGL((mt::lamb_apply_kernel<scalar_t>),
                               dim3(plan.n_blocks), dim3(256), 0, stream,
                               chunks, tab, lay, ratio, (float)lr, b1, omb1,
                               log_b1, b2, omb2, log_b2, (float)eps, step_p,
                               a.guard, a.lr);
          });
    });
  }
}

torch::Tensor l2norm_sq(std::vector<torch::Tensor> grads) {
  TORCH_CHECK(!grads.empty());
  auto dev = grads[0].device();
  auto out = torch::zeros({}, torch::dtype(torch::kFloat32).device(dev));
  PlanKey key;
  key.ptrs.reserve(2 * grads.size() + 2);
  key.ptrs.push_back((const void*)0x127);  // op tag
  key.ptrs.push_back((const void*)(uintptr_t)grads.size());
  for (auto& g : grads) {
    key.ptrs.push_back(g.data_ptr());
    key.ptrs.push_back((const void*)(uintptr_t)g.numel());
  }
  const auto& plans = cached_plans(std::move(key), [&] {
    return make_plans(grads, dev,
                      [&](size_t i, int local, mt::PtrTable* tab) {
                        tab->grad[local] = grads[i].data_ptr();
                      });
  });
  auto stream = c10::hip::getCurrentHIPStream();
  for (auto& plan : plans) {
    DDP_DISPATCH_FLOAT(grads[0].scalar_type(), "l2norm_sq", [&] {
      hipLaunchKernelGGL(
          (mt::l2norm_sq_kernel<scalar_t>), dim3(plan.n_blocks), dim3(256), 0,
          stream,
          reinterpret_cast<const mt::ChunkDesc*>(plan.chunks_dev.data_ptr()),
          reinterpret_cast<const mt::PtrTable*>(plan.table_dev.data_ptr()),
          out.data_ptr<float>());
    });
  }
  return out;
}

static void scale_impl(std::vector<torch::Tensor>& ts, float s,
                       const torch::Tensor* dev_scale, bool clamp) {
  auto dev = ts[0].device();
  PlanKey key;
  key.ptrs.reserve(2 * ts.size() + 2);
  key.ptrs.push_back((const void*)0x5CA1E);  // op tag
  key.ptrs.push_back((const void*)(uintptr_t)ts.size());
  for (auto& t : ts) {
    key.ptrs.push_back(t.data_ptr());
    key.ptrs.push_back((const void*)(uintptr_t)t.numel());
  }
  const auto& plans = cached_plans(std::move(key), [&] {
    return make_plans(ts, dev, [&](size_t i, int local, mt::PtrTable* tab) {
      tab->param[local] = ts[i].data_ptr();
    });
  });
  auto stream = c10::hip::getCurrentHIPStream();
  for (auto& plan : plans) {
    DDP_DISPATCH_FLOAT(ts[0].scalar_type(), "scale_", [&] {
      hipLaunchKernelGGL(
          (mt::scale_kernel<scalar_t>), dim3(plan.n_blocks), dim3(256), 0,
          stream,
          reinterpret_cast<const mt::ChunkDesc*>(plan.chunks_dev.data_ptr()),
          reinterpret_cast<const mt::PtrTable*>(plan.table_dev.data_ptr()), s,
          dev_scale ? dev_scale->data_ptr<float>() : nullptr, clamp ? 1 : 0);
    });
  }
}

void scale_(std::vector<torch::Tensor> ts, double s) {
  TORCH_CHECK(!ts.empty());
  scale_impl(ts, (float)s, nullptr, false);
}

void scale_by_tensor_(std::vector<torch::Tensor> ts, torch::Tensor s) {
  TORCH_CHECK(!ts.empty());
  TORCH_CHECK(s.scalar_type() == torch::kFloat32 && s.numel() == 1);
  scale_impl(ts, 1.f, &s, /*clamp=*/true);
}
