// Multi-tensor optimizer / gradient utilities (CDNA4, gfx950).
//
// Reference parity: SGD step (reference optim.SGD,
// ddp.py:183/240) as a fused multi-tensor kernel; global L2 grad norm +
// scale for clip_grad_norm_ (ddp.py:238-239).  Supports bf16 params with
// fp32 master weights (the apex-O2 slot, ddp.py:165-181, done natively).
// AdamW (the reference's apex FusedAdam slot) runs on the same
// machinery with its step count read from a device scalar.
//
// Chunking: tensor lists are flattened into fixed-size chunks dispatched to
// blocks through a device-side descriptor table, so one launch covers the
// whole parameter set regardless of tensor count.

#include <torch/extension.h>

#include <cmath>
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

}  // namespace mt

// ======================= host side =======================================

namespace {

struct LaunchPlan {
  torch::Tensor chunks_dev;   // ChunkDesc[]
  torch::Tensor table_dev;    // PtrTable
  torch::Tensor chunks_host;  // PINNED sources kept alive: a hipGraph-
  torch::Tensor table_host;   // captured H2D copy replays from this memory
  int n_blocks;
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
    plans.push_back(plan);
    t = t_end;
  }
  return plans;
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
