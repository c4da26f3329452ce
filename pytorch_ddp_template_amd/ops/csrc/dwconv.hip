// Depthwise conv2d on NHWC tensors (CDNA4, gfx950): forward, data gradient
// and weight gradient.  x [N,H,W,C]; w [C,R,R,1] (KRSC with one input channel
// per group); square R in {3, 5, 7}; stride 1; 0 <= pad <= R-1; C % 8 == 0.
// One template on the element type serves bf16, fp16 and fp32; every sum is
// fp32 and is rounded once at the store.
//
// Why no MFMA: the reduction runs over the R*R taps only and channels are the
// contiguous axis.  A per-channel banded-matrix product would need operands
// strided by C elements, i.e. a transposing gather per channel, which costs
// more than the VALU FMAs it replaces.  These are fp32 VALU kernels fed from
// LDS.
//
// A pixel's slab of 32 channels is 4 lanes x 8 channels ("octet", 16 B of a
// 16-bit type, 2 x 16 B of fp32).  The LDS patch is [row][col][4 lanes] octets
// with an ODD number of columns per row, so that the 4 lanes x 4 rows of 16
// neighbouring threads fall into different banks.
//
// fwd_kernel<T, R, TW, FLIP>: one block = one image, one 32-channel slab, one
// TH x TW tile of outputs.  The input patch (tile + R-1 halo) is staged once
// with zeros for out-of-image positions, the slab's R*R weights are staged
// tap-major (bit copies, reversed when FLIP), and each thread then makes a run
// of 4 adjacent outputs along W for its octet: per tap row 4+R-1 input octets
// and R weight octets from LDS for 4*R*8 FMAs.  Bounds are tested at the
// staging and at the store only.  The data gradient is this kernel with
// FLIP = true and pad' = R-1-pad.
//
// wgrad_kernel<T, R> + wgrad_reduce_kernel: a block walks tiles (image, row
// band, column band) of one slab, staging the x patch and the dy tile.  A
// thread owns (octet, tap row r, pixel-row group) and walks along W with a
// register window of R input octets: one new x octet and one dy octet per
// step for R*8 FMAs into R*8 accumulators.  The groups are summed through LDS
// in a fixed order, each block writes ONE fp32 partial [R*R, 32] into the
// workspace [blocks_per_slab, R*R, C], and the second kernel sums the
// partials in a fixed order.  No atomics: the result is repeatable.  At most
// kWgradBlockCap blocks run, so the workspace is at most
// kWgradBlockCap * 49 * 32 * 4 B = 6.1 MiB (C is held to 1024 slabs, which
// also keeps gridDim.y in range).
//
// All three take their memory from the caching allocator on the current
// stream and never synchronise, so they can be captured into a hipGraph.

#include <torch/extension.h>

#include <algorithm>
#include <cstdint>

#include "common.h"
#include "dispatch.h"

namespace dw {

constexpr int kSlab = 32;            // channels per block
constexpr int kWgradBlockCap = 1024; // wgrad blocks over all slabs
constexpr int kWgradThreads = 256;
constexpr int kReduceLanes = 8;      // partial sums per output in the reduce

// 8 channels of one pixel
template <typename T>
struct Oct {
  using IO = VecIO<T>;
  static constexpr int P = IO::kPerLane;
  static constexpr int NV = 8 / P;
  typename IO::Vec v[NV];

  DEV_INLINE void zero() {
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = (typename IO::Vec)(0);
  }
  DEV_INLINE void load(const T* p) {
#pragma unroll
    for (int i = 0; i < NV; ++i)
      v[i] = reinterpret_cast<const typename IO::Vec*>(p)[i];
  }
  DEV_INLINE void store(T* p) const {
#pragma unroll
    for (int i = 0; i < NV; ++i)
      reinterpret_cast<typename IO::Vec*>(p)[i] = v[i];
  }
  DEV_INLINE void unpack(float* f) const {
#pragma unroll
    for (int k = 0; k < 8; ++k) f[k] = IO::get(v[k / P], k % P);
  }
  DEV_INLINE void pack(const float* f) {
#pragma unroll
    for (int k = 0; k < 8; ++k) IO::set(v[k / P], k % P, f[k]);
  }
};

// Stage a PH x PW patch of `src` [.,SH,SW,C] (image n, rows from y0, columns
// from x0, channels from c0) into LDS [PH][PWS][4] octets, zeros outside.
template <typename T, int PH, int PW, int PWS, int THREADS>
DEV_INLINE void stage_patch(T* lds, const T* __restrict__ src, int n, int SH,
                            int SW, int C, int y0, int x0, int c0, int tid) {
  for (int i = tid; i < PH * PW * 4; i += THREADS) {
    const int cl = i & 3, pos = i >> 2;
    const int pr = pos / PW, pc = pos - pr * PW;
    const int iy = y0 + pr, ix = x0 + pc, c = c0 + cl * 8;
    Oct<T> o;
    if ((unsigned)iy < (unsigned)SH && (unsigned)ix < (unsigned)SW && c < C)
      o.load(src + (((long long)n * SH + iy) * SW + ix) * C + c);
    else
      o.zero();
    o.store(lds + ((pr * PWS + pc) * 4 + cl) * 8);
  }
}

template <typename T, int R, int TW>
struct FwdGeo {
  static constexpr int RUNS_X = TW / 4;
  // 64 runs of 4 outputs (16-bit) or 32 (fp32, whose patch is twice as big)
  static constexpr int TH = (sizeof(T) == 4 ? 32 : 64) / RUNS_X;
  static constexpr int THREADS = TH * RUNS_X * 4;
  static constexpr int PH = TH + R - 1, PW = TW + R - 1, PWS = PW | 1;
  static constexpr int PATCH = PH * PWS * kSlab;  // elements
  static constexpr int WTS = R * R * kSlab;
};

template <typename T, int R, int TW, bool FLIP>
__global__ NO_PK_F32 __launch_bounds__((FwdGeo<T, R, TW>::THREADS)) void
fwd_kernel(const T* __restrict__ x, const T* __restrict__ w,
           const T* __restrict__ bias, T* __restrict__ y, int H, int W, int C,
           int HO, int WO, int pad, int tiles_x, int slabs) {
  using G = FwdGeo<T, R, TW>;
  __shared__ __attribute__((aligned(16))) T patch[G::PATCH];
  __shared__ __attribute__((aligned(16))) T wl[G::WTS];
  const int tid = threadIdx.x;
  const int slab = blockIdx.x % slabs, tile = blockIdx.x / slabs;
  const int tile_y = tile / tiles_x, tile_x = tile - tile_y * tiles_x;
  const int n = blockIdx.y, c0 = slab * kSlab;
  const int oy0 = tile_y * G::TH, ox0 = tile_x * TW;

  stage_patch<T, G::PH, G::PW, G::PWS, G::THREADS>(
      patch, x, n, H, W, C, oy0 - pad, ox0 - pad, c0, tid);
  // weights [C, R*R] -> tap-major [R*R][32], reversed for the data gradient
  for (int i = tid; i < G::WTS; i += G::THREADS) {
    const int c = i / (R * R), t = i - c * (R * R);
    const int tl = FLIP ? R * R - 1 - t : t;
    T v = w[0];
    if (c0 + c < C) v = w[(long long)(c0 + c) * (R * R) + t];
    // a lane past C multiplies patch zeros; its result is never stored
    wl[tl * kSlab + c] = v;
  }
  __syncthreads();

  const int cl = tid & 3, ty = (tid >> 2) % G::TH, run = (tid >> 2) / G::TH;
  float acc[4][8];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[j][k] = 0.f;
  const T* prow = patch + ((ty * G::PWS + run * 4) * 4 + cl) * 8;
#pragma unroll 1
  for (int r = 0; r < R; ++r) {
    float xin[4 + R - 1][8];
#pragma unroll
    for (int k = 0; k < 4 + R - 1; ++k) {
      Oct<T> o;
      o.load(prow + (r * G::PWS + k) * kSlab);
      o.unpack(xin[k]);
    }
#pragma unroll
    for (int s = 0; s < R; ++s) {
      Oct<T> ow;
      float wv[8];
      ow.load(wl + ((r * R + s) * 4 + cl) * 8);
      ow.unpack(wv);
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int k = 0; k < 8; ++k)
          acc[j][k] = fmaf(xin[j + s][k], wv[k], acc[j][k]);
    }
  }

  const int oy = oy0 + ty, c = c0 + cl * 8;
  if (oy >= HO || c >= C) return;
  float bv[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) bv[k] = 0.f;
  if (bias != nullptr) {
    Oct<T> ob;
    ob.load(bias + c);
    ob.unpack(bv);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int ox = ox0 + run * 4 + j;
    if (ox >= WO) break;
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[j][k] += bv[k];
    Oct<T> o;
    o.pack(acc[j]);
    o.store(y + (((long long)n * HO + oy) * WO + ox) * C + c);
  }
}

template <typename T, int R>
struct WgGeo {
  static constexpr int TW = sizeof(T) == 4 ? 16 : 32;
  static constexpr int TH = R == 7 ? 8 : 10;
  static constexpr int NSEG = R == 3 ? 2 : 1;  // walks per tile row
  static constexpr int SEG = TW / NSEG;
  static constexpr int GROUPS = TH * NSEG;
  static_assert(4 * R * GROUPS <= kWgradThreads, "wgrad thread budget");
  static constexpr int PH = TH + R - 1, PW = TW + R - 1, PWS = PW | 1;
  static constexpr int XE = PH * PWS * kSlab;  // elements of the x patch
  static constexpr int DYE = TH * TW * kSlab;
  static constexpr int STAGE_B = (XE + DYE) * (int)sizeof(T);
  static constexpr int RED_B = GROUPS * R * R * kSlab * 4;
  static constexpr int SMEM_B = STAGE_B > RED_B ? STAGE_B : RED_B;
  static_assert(SMEM_B <= 65536, "wgrad LDS budget");
};

template <typename T, int R>
__global__ NO_PK_F32 __launch_bounds__(kWgradThreads) void wgrad_kernel(
    const T* __restrict__ dy, const T* __restrict__ x, float* __restrict__ ws,
    int H, int W, int C, int HO, int WO, int pad, int tiles_y, int tiles_x,
    int ntiles) {
  using G = WgGeo<T, R>;
  __shared__ __attribute__((aligned(16))) unsigned char smem[G::SMEM_B];
  T* xp = reinterpret_cast<T*>(smem);
  T* dyt = xp + G::XE;
  const int tid = threadIdx.x;
  const int c0 = blockIdx.y * kSlab;
  const int cl = tid & 3, r = (tid >> 2) % R, g = (tid >> 2) / R;
  const bool active = g < G::GROUPS;
  const int row = g / G::NSEG, s0 = (g % G::NSEG) * G::SEG;

  float acc[R][8];
#pragma unroll
  for (int s = 0; s < R; ++s)
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[s][k] = 0.f;

  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int tx = tile % tiles_x, rest = tile / tiles_x;
    const int ty = rest % tiles_y, n = rest / tiles_y;
    const int oy0 = ty * G::TH, ox0 = tx * G::TW;
    __syncthreads();  // the previous tile has been read
    stage_patch<T, G::PH, G::PW, G::PWS, kWgradThreads>(
        xp, x, n, H, W, C, oy0 - pad, ox0 - pad, c0, tid);
    stage_patch<T, G::TH, G::TW, G::TW, kWgradThreads>(dyt, dy, n, HO, WO, C,
                                                        oy0, ox0, c0, tid);
    __syncthreads();
    const int th = min(G::TH, HO - oy0);
    const int len = min(G::SEG, WO - ox0 - s0);
    if (active && row < th && len > 0) {
      const T* xrow = xp + (((row + r) * G::PWS + s0) * 4 + cl) * 8;
      const T* drow = dyt + ((row * G::TW + s0) * 4 + cl) * 8;
      // window slot of patch column s0 + c is c % R
      float win[R][8];
#pragma unroll
      for (int c = 0; c < R - 1; ++c) {
        Oct<T> o;
        o.load(xrow + c * kSlab);
        o.unpack(win[c]);
      }
      for (int base = 0; base < len; base += R) {
#pragma unroll
        for (int uu = 0; uu < R; ++uu) {
          const int u = base + uu;
          if (u < len) {
            Oct<T> o, od;
            float dv[8];
            o.load(xrow + (u + R - 1) * kSlab);
            o.unpack(win[(uu + R - 1) % R]);
            od.load(drow + u * kSlab);
            od.unpack(dv);
#pragma unroll
            for (int s = 0; s < R; ++s)
#pragma unroll
              for (int k = 0; k < 8; ++k)
                acc[s][k] = fmaf(dv[k], win[(uu + s) % R][k], acc[s][k]);
          }
        }
      }
    }
  }

  // groups -> one partial per block, in a fixed order
  __syncthreads();
  float* red = reinterpret_cast<float*>(smem);  // [GROUPS][R*R][32]
  if (active) {
#pragma unroll
    for (int s = 0; s < R; ++s)
#pragma unroll
      for (int k = 0; k < 8; ++k)
        red[(g * R * R + r * R + s) * kSlab + cl * 8 + k] = acc[s][k];
  }
  __syncthreads();
  for (int i = tid; i < R * R * kSlab; i += kWgradThreads) {
    const int c = c0 + (i & (kSlab - 1));
    float sum = 0.f;
    for (int gg = 0; gg < G::GROUPS; ++gg) sum += red[gg * R * R * kSlab + i];
    if (c < C)
      ws[((long long)blockIdx.x * (R * R) + (i / kSlab)) * C + c] = sum;
  }
}

// ws [nb, RR, C] -> dw [C, RR]: block (t, slab); 8 lanes per channel each sum
// every 8th partial in order, then the 8 are summed in order.
__global__ NO_PK_F32 __launch_bounds__(kSlab* kReduceLanes) void
wgrad_reduce_kernel(const float* __restrict__ ws, float* __restrict__ dw,
                    int nb, int RR, int C) {
  __shared__ float part[kReduceLanes][kSlab];
  const int t = blockIdx.x, cc = threadIdx.x & (kSlab - 1);
  const int lane = threadIdx.x / kSlab, c = blockIdx.y * kSlab + cc;
  float sum = 0.f;
  if (c < C)
    for (int b = lane; b < nb; b += kReduceLanes)
      sum += ws[((long long)b * RR + t) * C + c];
  part[lane][cc] = sum;
  __syncthreads();
  if (lane == 0 && c < C) {
    float tot = 0.f;
#pragma unroll
    for (int l = 0; l < kReduceLanes; ++l) tot += part[l][cc];
    dw[(long long)c * RR + t] = tot;
  }
}

}  // namespace dw

// ======================= host launchers ==================================

namespace {

inline bool aligned16(const torch::Tensor& t) {
  return (reinterpret_cast<uintptr_t>(t.data_ptr()) & 15u) == 0;
}

struct Shape {
  int N, H, W, C, R, pad, HO, WO;
};

// a [N,H,W,C] tensor and the taps: everything the kernels assume
void check_common(const char* name, const torch::Tensor& a, int64_t R,
                  int64_t pad) {
  TORCH_CHECK(a.is_cuda() && a.dim() == 4 && a.is_contiguous(), name,
              ": expected a contiguous [N,H,W,C] GPU tensor");
  TORCH_CHECK(a.size(3) % 8 == 0, name, ": C must be a multiple of 8, got ",
              a.size(3));
  TORCH_CHECK(R == 3 || R == 5 || R == 7, name,
              ": square taps of 3, 5 or 7 only, got ", R);
  TORCH_CHECK(pad >= 0 && pad <= R - 1, name, ": pad must be in [0, R-1], got ",
              pad);
  TORCH_CHECK(a.size(0) >= 1 && a.size(0) <= 65535, name,
              ": batch must be in [1, 65535]");
  TORCH_CHECK(aligned16(a), name, ": tensors must be 16-byte aligned");
  // 1024 slabs: one wgrad block per slab at the cap, and gridDim.y in range
  TORCH_CHECK(a.size(3) <= dw::kWgradBlockCap * dw::kSlab, name,
              ": at most ", dw::kWgradBlockCap * dw::kSlab, " channels");
  TORCH_CHECK(a.size(1) >= 1 && a.size(2) >= 1, name, ": empty map ",
              a.sizes());
}

void check_weight(const char* name, const torch::Tensor& w,
                  const torch::Tensor& a) {
  TORCH_CHECK(w.is_cuda() && w.is_contiguous() && w.dim() == 4 &&
                  w.size(0) == a.size(3) && w.size(1) == w.size(2) &&
                  w.size(3) == 1 && w.scalar_type() == a.scalar_type() &&
                  w.device() == a.device(),
              name, ": w must be a contiguous [C,R,R,1] tensor of x's dtype");
}

template <typename T, int R, int TW, bool FLIP>
void launch_fwd_tw(const torch::Tensor& x, const torch::Tensor& w,
                   const torch::Tensor* bias, torch::Tensor& y, const Shape& s,
                   int pad) {
  using G = dw::FwdGeo<T, R, TW>;
  const int tiles_x = (s.WO + TW - 1) / TW, tiles_y = (s.HO + G::TH - 1) / G::TH;
  const int slabs = (s.C + dw::kSlab - 1) / dw::kSlab;
  const long long gx = (long long)tiles_x * tiles_y * slabs;
  TORCH_CHECK(gx <= 0x7fffffffLL, "dwconv2d: map too large");
  hipLaunchKernelGGL((dw::fwd_kernel<T, R, TW, FLIP>),
                     dim3((unsigned)gx, (unsigned)s.N), dim3(G::THREADS), 0,
                     c10::hip::getCurrentHIPStream(),
                     reinterpret_cast<const T*>(x.data_ptr()),
                     reinterpret_cast<const T*>(w.data_ptr()),
                     bias ? reinterpret_cast<const T*>(bias->data_ptr())
                          : nullptr,
                     reinterpret_cast<T*>(y.data_ptr()), s.H, s.W, s.C, s.HO,
                     s.WO, pad, tiles_x, slabs);
}

template <typename T, bool FLIP>
void launch_fwd(const torch::Tensor& x, const torch::Tensor& w,
                const torch::Tensor* bias, torch::Tensor& y, const Shape& s,
                int pad) {
  // narrow maps take the 16-wide tile (a 14-wide map fills 7/8 of it)
#define DW_FWD(RR)                                                  \
  if (s.WO <= 16)                                                   \
    launch_fwd_tw<T, RR, 16, FLIP>(x, w, bias, y, s, pad);          \
  else                                                              \
    launch_fwd_tw<T, RR, 32, FLIP>(x, w, bias, y, s, pad);          \
  break;
  switch (s.R) {
    case 3: DW_FWD(3)
    case 5: DW_FWD(5)
    default: DW_FWD(7)
  }
#undef DW_FWD
}

template <typename T, int R>
void launch_wgrad(const torch::Tensor& dy, const torch::Tensor& x,
                  torch::Tensor& out, const Shape& s) {
  using G = dw::WgGeo<T, R>;
  const int tiles_x = (s.WO + G::TW - 1) / G::TW;
  const int tiles_y = (s.HO + G::TH - 1) / G::TH;
  const long long ntiles = (long long)s.N * tiles_y * tiles_x;
  TORCH_CHECK(ntiles <= 0x7fffffffLL, "dwconv2d_wgrad: map too large");
  const int slabs = (s.C + dw::kSlab - 1) / dw::kSlab;
  const int nb = (int)std::min<long long>(
      ntiles, std::max(1, dw::kWgradBlockCap / slabs));
  auto ws = torch::empty({nb, R * R, s.C}, out.options());
  auto stream = c10::hip::getCurrentHIPStream();
  hipLaunchKernelGGL((dw::wgrad_kernel<T, R>), dim3(nb, slabs),
                     dim3(dw::kWgradThreads), 0, stream,
                     reinterpret_cast<const T*>(dy.data_ptr()),
                     reinterpret_cast<const T*>(x.data_ptr()),
                     ws.data_ptr<float>(), s.H, s.W, s.C, s.HO, s.WO, s.pad,
                     tiles_y, tiles_x, (int)ntiles);
  hipLaunchKernelGGL(dw::wgrad_reduce_kernel, dim3(R * R, slabs),
                     dim3(dw::kSlab * dw::kReduceLanes), 0, stream,
                     ws.data_ptr<float>(), out.data_ptr<float>(), nb, R * R,
                     s.C);
}

}  // namespace

int64_t dwconv_wgrad_block_cap() { return dw::kWgradBlockCap; }

// y[n,oy,ox,c] = bias[c] + sum_{r,s} x[n,oy-pad+r,ox-pad+s,c] * w[c,r,s]
torch::Tensor dwconv2d_fwd(torch::Tensor x, torch::Tensor w,
                           c10::optional<torch::Tensor> bias, int64_t pad) {
  TORCH_CHECK(w.dim() == 4, "dwconv2d_fwd: w must be [C,R,R,1]");
  const int64_t R = w.size(1);
  check_common("dwconv2d_fwd", x, R, pad);
  check_weight("dwconv2d_fwd", w, x);
  Shape s{(int)x.size(0), (int)x.size(1), (int)x.size(2), (int)x.size(3),
          (int)R,         (int)pad,       0,              0};
  s.HO = s.H + 2 * s.pad - s.R + 1;
  s.WO = s.W + 2 * s.pad - s.R + 1;
  TORCH_CHECK(s.HO >= 1 && s.WO >= 1, "dwconv2d_fwd: empty output");
  const torch::Tensor* bp = nullptr;
  if (bias.has_value()) {
    TORCH_CHECK(bias->is_cuda() && bias->is_contiguous() &&
                    bias->numel() == s.C && aligned16(*bias) &&
                    bias->scalar_type() == x.scalar_type() &&
                    bias->device() == x.device(),
                "dwconv2d_fwd: bias must be [C] of x's dtype");
    bp = &*bias;
  }
  auto y = torch::empty({s.N, s.HO, s.WO, s.C}, x.options());
  DDP_DISPATCH_FLOAT(x.scalar_type(), "dwconv2d_fwd", [&] {
    launch_fwd<scalar_t, false>(x, w, bp, y, s, s.pad);
  });
  return y;
}

// dx[n,iy,ix,c] = sum_{r,s} dy[n,iy+pad-r,ix+pad-s,c] * w[c,r,s]: the forward
// kernel over dy with the taps reversed and pad' = R-1-pad
torch::Tensor dwconv2d_dgrad(torch::Tensor dy, torch::Tensor w, int64_t pad,
                             int64_t H, int64_t W) {
  TORCH_CHECK(w.dim() == 4, "dwconv2d_dgrad: w must be [C,R,R,1]");
  const int64_t R = w.size(1);
  check_common("dwconv2d_dgrad", dy, R, pad);
  check_weight("dwconv2d_dgrad", w, dy);
  TORCH_CHECK(H >= 1 && W >= 1, "dwconv2d_dgrad: empty dx");
  TORCH_CHECK(dy.size(1) == H + 2 * pad - R + 1 &&
                  dy.size(2) == W + 2 * pad - R + 1,
              "dwconv2d_dgrad: dy does not match H, W, pad");
  // the kernel's "input" is dy and its "output" is dx
  Shape s{(int)dy.size(0), (int)dy.size(1), (int)dy.size(2), (int)dy.size(3),
          (int)R,          (int)pad,        (int)H,          (int)W};
  auto dx = torch::empty({s.N, H, W, s.C}, dy.options());
  DDP_DISPATCH_FLOAT(dy.scalar_type(), "dwconv2d_dgrad", [&] {
    launch_fwd<scalar_t, true>(dy, w, nullptr, dx, s, s.R - 1 - s.pad);
  });
  return dx;
}

// dw[c,r,s] = sum_{n,oy,ox} dy[n,oy,ox,c] * x[n,oy-pad+r,ox-pad+s,c], fp32
torch::Tensor dwconv2d_wgrad(torch::Tensor dy, torch::Tensor x, int64_t pad,
                             int64_t R) {
  check_common("dwconv2d_wgrad", x, R, pad);
  check_common("dwconv2d_wgrad", dy, R, pad);
  TORCH_CHECK(dy.scalar_type() == x.scalar_type() &&
                  dy.device() == x.device() && dy.size(0) == x.size(0) &&
                  dy.size(3) == x.size(3) &&
                  dy.size(1) == x.size(1) + 2 * pad - R + 1 &&
                  dy.size(2) == x.size(2) + 2 * pad - R + 1,
              "dwconv2d_wgrad: dy does not match x, pad, R");
  Shape s{(int)x.size(0),  (int)x.size(1), (int)x.size(2), (int)x.size(3),
          (int)R,          (int)pad,       (int)dy.size(1), (int)dy.size(2)};
  auto out = torch::empty({s.C, R, R, 1},
                          x.options().dtype(torch::kFloat32));
  DDP_DISPATCH_FLOAT(x.scalar_type(), "dwconv2d_wgrad", [&] {
    switch (s.R) {
      case 3: launch_wgrad<scalar_t, 3>(dy, x, out, s); break;
      case 5: launch_wgrad<scalar_t, 5>(dy, x, out, s); break;
      default: launch_wgrad<scalar_t, 7>(dy, x, out, s); break;
    }
  });
  return out;
}
