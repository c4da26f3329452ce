// Loss kernels (CDNA4, gfx950).
//
// * Fused cross-entropy: log-softmax + NLL in one pass (mean reduction),
//   saving the row logsumexp for a one-pass backward — the op BASELINE.json
//   names for the classification configs.
// * MSE — the reference template's criterion (reference ddp.py:164,222).
//
// Backward kernels read the incoming dLoss as a DEVICE scalar so the train
// loop never syncs the host on loss readback (SURVEY.md §3.2 calls out the
// reference's per-step loss.item() stall).

#include <torch/extension.h>

#include "common.h"
#include "dispatch.h"

namespace loss {

// one block per row: lse + per-row loss contribution (atomic mean)
template <typename T>
__global__ void ce_fwd_kernel(const T* __restrict__ logits,
                              const int64_t* __restrict__ target,
                              float* __restrict__ loss_out,
                              float* __restrict__ lse_out, int D) {
  __shared__ float lds[4];
  const long long m = blockIdx.x;
  const T* row = logits + m * D;
  float mx = -INFINITY;
  for (int d = threadIdx.x; d < D; d += blockDim.x)
    mx = fmaxf(mx, to_f(row[d]));
  float wmax = wave_reduce_max(mx);
  if (lane_id() == 0) lds[wave_id()] = wmax;
  __syncthreads();
  float bmax = fmaxf(fmaxf(lds[0], lds[1]), fmaxf(lds[2], lds[3]));
  __syncthreads();
  float s = 0.f;
  for (int d = threadIdx.x; d < D; d += blockDim.x)
    s += __expf(to_f(row[d]) - bmax);
  s = block_reduce_sum<256>(s, lds);
  if (threadIdx.x == 0) {
    const float lse = bmax + __logf(s);
    lse_out[m] = lse;
    const float nll = lse - to_f(row[target[m]]);
    atomicAdd(loss_out, nll / (float)gridDim.x);  // mean over rows
  }
}

// dlogits = (softmax - onehot) * (dloss / M); dloss read on device
template <typename T>
__global__ void ce_bwd_kernel(const T* __restrict__ logits,
                              const int64_t* __restrict__ target,
                              const float* __restrict__ lse,
                              const float* __restrict__ dloss,
                              T* __restrict__ dlogits, long long M, int D) {
  const float scale = dloss[0] / (float)M;
  const long long total = M * D;
  GRID_STRIDE(i, total) {
    const long long m = i / D;
    const int d = (int)(i % D);
    float sm = __expf(to_f(logits[i]) - lse[m]);
    if ((long long)d == target[m]) sm -= 1.f;
    dlogits[i] = to_t<T>(sm * scale);
  }
}

// mse: mean((p - t)^2); partial sums via block reduce + atomic
template <typename T>
__global__ void mse_fwd_kernel(const T* __restrict__ p, const T* __restrict__ t,
                               float* __restrict__ out, long long n) {
  __shared__ float lds[4];
  float acc = 0.f;
  GRID_STRIDE(i, n) {
    float d = to_f(p[i]) - to_f(t[i]);
    acc += d * d;
  }
  float total = block_reduce_sum<256>(acc, lds);
  if (threadIdx.x == 0) atomicAdd(out, total / (float)n);
}

template <typename T>
__global__ void mse_bwd_kernel(const T* __restrict__ p, const T* __restrict__ t,
                               const float* __restrict__ dloss,
                               T* __restrict__ dp, long long n) {
  const float scale = 2.f * dloss[0] / (float)n;
  GRID_STRIDE(i, n) {
    dp[i] = to_t<T>(scale * (to_f(p[i]) - to_f(t[i])));
  }
}

// ---- soft-target cross-entropy: label smoothing + mixup / cutmix labels ----
//
// The target distribution of row m is never built:
//   q_d = eps/D + (1 - eps) (lam [d == t_m] + (1 - lam) [d == t_{M-1-m}])
// with the partner row M-1-m of the batch flip of mix.hip and lam = slot 0 of
// the mix params record, read on the device (null record: lam = 1, plain
// label smoothing).  Since sum_d q_d = 1 the row loss is
//   lse - (1 - eps) (lam z_ta + (1 - lam) z_tb) - (eps/D) sum_d z_d .
// Forward and backward of one step read the SAME record: the only thing that
// writes it is the next step's draw (BatchMix.apply_), which runs before that
// step's forward, so nothing saves a private copy of lam.

struct SoftStat {
  float mx, s, sz;  // running max, sum exp(z - mx), sum z
};

// exp(m_i - m) with an empty part (m_i = -inf) contributing nothing
DEV_INLINE float rescale(float mi, float m) {
  return mi == -INFINITY ? 0.f : __expf(mi - m);
}

DEV_INLINE void soft_merge(SoftStat& a, float mx, float s, float sz) {
  const float m = fmaxf(a.mx, mx);
  a.s = a.s * rescale(a.mx, m) + s * rescale(mx, m);
  a.sz += sz;
  a.mx = m;
}

DEV_INLINE float soft_q(int d, int ta, int tb, float base, float wa,
                        float wb) {
  return base + (d == ta ? wa : 0.f) + (d == tb ? wb : 0.f);
}

// Row per wave, four rows per 256-thread block.  The row is read ONCE: each
// lane keeps an online (max, sumexp) pair and a running sum z over its 16-byte
// vectors, the 64 triples are merged with shuffles (rescale on merge), and
// lane 0 finishes the row.  No LDS, no barrier, so the waves of a partial
// last block just leave.  vec == 0: rows that do not start on 16-byte
// boundaries are read element by element.
template <typename T>
__global__ NO_PK_F32 void ce_soft_fwd_kernel(
    const T* __restrict__ logits, const int64_t* __restrict__ target,
    const float* __restrict__ mixrec, float* __restrict__ loss_out,
    float* __restrict__ lse_out, int M, int D, float eps, int vec) {
  using IO = VecIO<T>;
  constexpr int P = IO::kPerLane;
  const int m = blockIdx.x * 4 + wave_id();
  if (m >= M) return;
  const int lane = lane_id();
  const T* row = logits + (long long)m * D;
  SoftStat st = {-INFINITY, 0.f, 0.f};
  if (vec) {
    const auto* vrow = reinterpret_cast<const typename IO::Vec*>(row);
    for (int v = lane; v < D / P; v += kWave) {
      const typename IO::Vec x = vrow[v];
      float z[P], vmx = -INFINITY, vsz = 0.f, vs = 0.f;
#pragma unroll
      for (int j = 0; j < P; ++j) {
        z[j] = IO::get(x, j);
        vmx = fmaxf(vmx, z[j]);
        vsz += z[j];
      }
      const float mnew = fmaxf(st.mx, vmx);
#pragma unroll
      for (int j = 0; j < P; ++j) vs += __expf(z[j] - mnew);
      st.s = st.s * rescale(st.mx, mnew) + vs;
      st.sz += vsz;
      st.mx = mnew;
    }
  } else {
    for (int d = lane; d < D; d += kWave) {
      const float z = to_f(row[d]);
      const float mnew = fmaxf(st.mx, z);
      st.s = st.s * rescale(st.mx, mnew) + __expf(z - mnew);
      st.sz += z;
      st.mx = mnew;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    soft_merge(st, __shfl_xor(st.mx, off), __shfl_xor(st.s, off),
               __shfl_xor(st.sz, off));
  if (lane != 0) return;
  const float lse = st.mx + __logf(st.s);
  lse_out[m] = lse;
  const float lam = mixrec ? mixrec[0] : 1.f;
  const long long ta = target[m], tb = target[M - 1 - m];
  const float za = (unsigned long long)ta < (unsigned long long)D
                       ? to_f(row[ta]) : 0.f;
  const float zb = (unsigned long long)tb < (unsigned long long)D
                       ? to_f(row[tb]) : 0.f;
  const float loss = lse - (1.f - eps) * (lam * za + (1.f - lam) * zb) -
                     (eps / (float)D) * st.sz;
  atomicAdd(loss_out, loss / (float)M);  // mean over rows
}

// dlogits = (exp(z - lse) - q) * (dloss / M); dloss and lam read on device.
// One 16-byte vector per work item when rows are whole vectors, else one
// element; capped grid, grid-stride.
template <typename T, bool VEC>
__global__ NO_PK_F32 void ce_soft_bwd_kernel(
    const T* __restrict__ logits, const int64_t* __restrict__ target,
    const float* __restrict__ lse, const float* __restrict__ dloss,
    const float* __restrict__ mixrec, T* __restrict__ dlogits, int M, int D,
    float eps) {
  using IO = VecIO<T>;
  constexpr int P = VEC ? IO::kPerLane : 1;
  const float scale = dloss[0] / (float)M;
  const float lam = mixrec ? mixrec[0] : 1.f;
  const float base = eps / (float)D;
  const float wa = (1.f - eps) * lam, wb = (1.f - eps) * (1.f - lam);
  const int per = D / P;  // work items per row
  const long long total = (long long)M * per;
  GRID_STRIDE(i, total) {
    const int m = (int)(i / per);
    const int d0 = (int)(i - (long long)m * per) * P;
    const int ta = (int)target[m], tb = (int)target[M - 1 - m];
    const float l = lse[m];
    const long long e = (long long)m * D + d0;
    if (VEC) {
      const typename IO::Vec x =
          *reinterpret_cast<const typename IO::Vec*>(logits + e);
      typename IO::Vec o;
#pragma unroll
      for (int j = 0; j < IO::kPerLane; ++j)
        IO::set(o, j, (__expf(IO::get(x, j) - l) -
                       soft_q(d0 + j, ta, tb, base, wa, wb)) * scale);
      *reinterpret_cast<typename IO::Vec*>(dlogits + e) = o;
    } else {
      dlogits[e] = to_t<T>((__expf(to_f(logits[e]) - l) -
                            soft_q(d0, ta, tb, base, wa, wb)) * scale);
    }
  }
}

}  // namespace loss

// ======================= host launchers ==================================

std::vector<torch::Tensor> ce_fwd(torch::Tensor logits, torch::Tensor target) {
  TORCH_CHECK(logits.dim() == 2 && logits.is_contiguous());
  TORCH_CHECK(target.scalar_type() == torch::kInt64);
  long long M = logits.size(0);
  int D = (int)logits.size(1);
  auto f32 = logits.options().dtype(torch::kFloat32);
  auto out = torch::zeros({}, f32);
  auto lse = torch::empty({M}, f32);
  auto stream = c10::hip::getCurrentHIPStream();
  DDP_DISPATCH_FLOAT(logits.scalar_type(), "ce_fwd", [&] {
    hipLaunchKernelGGL((loss::ce_fwd_kernel<scalar_t>), dim3((unsigned)M),
                       dim3(256), 0, stream,
                       reinterpret_cast<const scalar_t*>(logits.data_ptr()),
                       target.data_ptr<int64_t>(), out.data_ptr<float>(),
                       lse.data_ptr<float>(), D);
  });
  return {out, lse};
}

torch::Tensor ce_bwd(torch::Tensor logits, torch::Tensor target,
                     torch::Tensor lse, torch::Tensor dloss) {
  long long M = logits.size(0);
  int D = (int)logits.size(1);
  auto dl = torch::empty_like(logits);
  auto stream = c10::hip::getCurrentHIPStream();
  auto dloss_f = dloss.to(torch::kFloat32);
  DDP_DISPATCH_FLOAT(logits.scalar_type(), "ce_bwd", [&] {
    hipLaunchKernelGGL((loss::ce_bwd_kernel<scalar_t>),
                       dim3(grid_1d(M * D, 256)), dim3(256), 0, stream,
                       reinterpret_cast<const scalar_t*>(logits.data_ptr()),
                       target.data_ptr<int64_t>(), lse.data_ptr<float>(),
                       dloss_f.data_ptr<float>(),
                       reinterpret_cast<scalar_t*>(dl.data_ptr()), M, D);
  });
  return dl;
}

torch::Tensor mse_fwd(torch::Tensor p, torch::Tensor t) {
  long long n = p.numel();
  auto out = torch::zeros({}, p.options().dtype(torch::kFloat32));
  auto stream = c10::hip::getCurrentHIPStream();
  DDP_DISPATCH_FLOAT(p.scalar_type(), "mse_fwd", [&] {
    hipLaunchKernelGGL((loss::mse_fwd_kernel<scalar_t>),
                       dim3(grid_1d(n, 256)), dim3(256), 0, stream,
                       reinterpret_cast<const scalar_t*>(p.data_ptr()),
                       reinterpret_cast<const scalar_t*>(t.data_ptr()),
                       out.data_ptr<float>(), n);
  });
  return out;
}

torch::Tensor mse_bwd(torch::Tensor p, torch::Tensor t, torch::Tensor dloss) {
  long long n = p.numel();
  auto dp = torch::empty_like(p);
  auto stream = c10::hip::getCurrentHIPStream();
  auto dloss_f = dloss.to(torch::kFloat32);
  DDP_DISPATCH_FLOAT(p.scalar_type(), "mse_bwd", [&] {
    hipLaunchKernelGGL((loss::mse_bwd_kernel<scalar_t>),
                       dim3(grid_1d(n, 256)), dim3(256), 0, stream,
                       reinterpret_cast<const scalar_t*>(p.data_ptr()),
                       reinterpret_cast<const scalar_t*>(t.data_ptr()),
                       dloss_f.data_ptr<float>(),
                       reinterpret_cast<scalar_t*>(dp.data_ptr()), n);
  });
  return dp;
}

// ---- soft-target cross-entropy (label smoothing, mixup / cutmix labels) ---

namespace {

const float* soft_record(const c10::optional<torch::Tensor>& mix,
                         const torch::Tensor& logits, const char* who) {
  if (!mix.has_value()) return nullptr;
  TORCH_CHECK(mix->is_cuda() && mix->is_contiguous() &&
                  mix->scalar_type() == torch::kFloat32 &&
                  mix->numel() == 8 && mix->device() == logits.device(),
              who, ": the mix params must be a contiguous float32 tensor of 8 "
              "slots on the logits' device");
  return mix->data_ptr<float>();
}

void soft_check(const torch::Tensor& logits, const torch::Tensor& target,
                double eps, const char* who) {
  TORCH_CHECK(logits.is_cuda() && logits.dim() == 2 && logits.is_contiguous(),
              who, ": logits must be a contiguous [M, D] GPU tensor");
  TORCH_CHECK(target.scalar_type() == torch::kInt64 && target.is_cuda() &&
                  target.is_contiguous() && target.dim() == 1 &&
                  target.size(0) == logits.size(0),
              who, ": target must be a contiguous int64 [M] GPU tensor");
  TORCH_CHECK(eps >= 0.0 && eps < 1.0, who, ": label smoothing ", eps,
              " not in [0, 1)");
  TORCH_CHECK(logits.size(0) >= 1 && logits.size(1) >= 1 &&
                  logits.size(0) < (1LL << 31) && logits.size(1) < (1LL << 31),
              who, ": M and D must be in [1, 2^31)");
}

// rows are whole 16-byte vectors and every row starts on a 16-byte boundary
template <typename T>
bool soft_vec_ok(const void* p, long long D) {
  return D % VecIO<T>::kPerLane == 0 &&
         (reinterpret_cast<uintptr_t>(p) & 15u) == 0;
}

}  // namespace

// returns {mean loss (f32 scalar), lse [M] f32}; mix: the 8-slot record of
// mix.hip whose slot 0 is lam, or None for lam = 1
std::vector<torch::Tensor> ce_soft_fwd(torch::Tensor logits,
                                       torch::Tensor target, double eps,
                                       c10::optional<torch::Tensor> mix) {
  soft_check(logits, target, eps, "ce_soft_fwd");
  const float* rec = soft_record(mix, logits, "ce_soft_fwd");
  const int M = (int)logits.size(0), D = (int)logits.size(1);
  auto f32 = logits.options().dtype(torch::kFloat32);
  auto out = torch::zeros({}, f32);
  auto lse = torch::empty({M}, f32);
  auto stream = c10::hip::getCurrentHIPStream();
  DDP_DISPATCH_FLOAT(logits.scalar_type(), "ce_soft_fwd", [&] {
    const int vec = soft_vec_ok<scalar_t>(logits.data_ptr(), D) ? 1 : 0;
    hipLaunchKernelGGL((loss::ce_soft_fwd_kernel<scalar_t>),
                       dim3((unsigned)((M + 3) / 4)), dim3(256), 0, stream,
                       reinterpret_cast<const scalar_t*>(logits.data_ptr()),
                       target.data_ptr<int64_t>(), rec, out.data_ptr<float>(),
                       lse.data_ptr<float>(), M, D, (float)eps, vec);
  });
  return {out, lse};
}

torch::Tensor ce_soft_bwd(torch::Tensor logits, torch::Tensor target,
                          torch::Tensor lse, torch::Tensor dloss, double eps,
                          c10::optional<torch::Tensor> mix) {
  soft_check(logits, target, eps, "ce_soft_bwd");
  const float* rec = soft_record(mix, logits, "ce_soft_bwd");
  const int M = (int)logits.size(0), D = (int)logits.size(1);
  TORCH_CHECK(lse.is_cuda() && lse.is_contiguous() &&
                  lse.scalar_type() == torch::kFloat32 && lse.numel() == M,
              "ce_soft_bwd: lse must be the forward's float32 [M] tensor");
  TORCH_CHECK(dloss.is_cuda() && dloss.numel() == 1,
              "ce_soft_bwd: dloss must be a one-element GPU tensor");
  auto dl = torch::empty_like(logits);
  auto stream = c10::hip::getCurrentHIPStream();
  auto dloss_f = dloss.to(torch::kFloat32);
  DDP_DISPATCH_FLOAT(logits.scalar_type(), "ce_soft_bwd", [&] {
    const bool vec = soft_vec_ok<scalar_t>(logits.data_ptr(), D) &&
                     soft_vec_ok<scalar_t>(dl.data_ptr(), D);
    const long long work =
        (long long)M * (vec ? D / VecIO<scalar_t>::kPerLane : D);
    const dim3 grid(grid_1d(work, 256)), block(256);
    auto* zp = reinterpret_cast<const scalar_t*>(logits.data_ptr());
    auto* dp = reinterpret_cast<scalar_t*>(dl.data_ptr());
    if (vec)
      hipLaunchKernelGGL((loss::ce_soft_bwd_kernel<scalar_t, true>), grid,
                         block, 0, stream, zp, target.data_ptr<int64_t>(),
                         lse.data_ptr<float>(), dloss_f.data_ptr<float>(), rec,
                         dp, M, D, (float)eps);
    else
      hipLaunchKernelGGL((loss::ce_soft_bwd_kernel<scalar_t, false>), grid,
                         block, 0, stream, zp, target.data_ptr<int64_t>(),
                         lse.data_ptr<float>(), dloss_f.data_ptr<float>(), rec,
                         dp, M, D, (float)eps);
  });
  return dl;
}
