// Large plain NT GEMM — 256x256 tile, glds-staged, CDNA4 (gfx950).
//
// C[M,N] = A[M,K] @ B[N,K]^T (+bias, +relu), bf16.  This is the big-shape
// path for the ViT linear layers (reference model.py:11,13 scope — SURVEY
// §2b GEMM row): M=50432, K/N in {768, 2304, 3072}.  Round 1 conceded these
// shapes to rocBLAS (846-1097 TF vs 510-687 TF for the 128-tile NT kernel);
// this kernel exists to close that gap and retire the library route.
//
// Structure (the verified 256² glds recipe from the CDNA4 guide):
//   * 256x256 macro-tile, BK=64, 8 waves as 2(M)x4(N), 512 threads.
//   * mfma_f32_16x16x32_bf16: per-wave 128x64 output = acc[8][4] f32x4.
//   * Staging via __builtin_amdgcn_global_load_lds (16B, wave-uniform LDS
//     base + lane*16): the LDS image IS the global access order, so both
//     operands land row-major [row][64k] — 128 KiB total, 2 buffers,
//     1 block/CU.
//   * One __syncthreads() per K-tile: the next tile's 8 glds are issued
//     BEFORE the current tile's MFMAs, so their latency hides under the
//     64 MFMAs; the barrier's implicit vmcnt(0) drains them after.
//   * Epilogue: accumulators staged through LDS (reusing the operand
//     buffers) so C is written in coalesced 16B rows.
// The K-slot XOR swizzle (T2) is applied on the glds SOURCE address with
// the matching XOR on the ds_read side: rows 4..7 (mod 8) swap 32B halves
// of each 64B k-span, taking the b128 fragment reads from 8-way to 4-way
// bank conflicts without touching the lane-linear LDS image.

#include <torch/extension.h>

#include "common.h"
#include "dispatch.h"

namespace gp {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int BM = 256, BN = 256, BK = 64;
constexpr int THREADS = 512;
constexpr int NT_BUF = 2;

__device__ __forceinline__ f32x4 mfma16(bf16x8 a, bf16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// K-slot swizzle: XOR the 32B half-slot of the 128B LDS row with bit 2 of
// the row (st_16x32: byte ^= ((byte>>9)&1)<<5 — row*128 puts row-bit-2 at
// byte-bit-9).  Applied to the glds *source* k-chunk and to ds_read
// addresses; the LDS image itself stays lane-linear.
__device__ __forceinline__ int kswz(int row, int kbyte) {
  return kbyte ^ (((row >> 2) & 1) << 5);
}

template <bool HAS_BIAS, bool RELU>
__global__ __launch_bounds__(THREADS, 1) void gemm_nt_plain256_kernel(
    const __hip_bfloat16* __restrict__ A, const __hip_bfloat16* __restrict__ B,
    __hip_bfloat16* __restrict__ C, const __hip_bfloat16* __restrict__ bias,
    int M, int N, int K) {
  // one shared object only (hipcc de-pipelines glds with a second one)
  __shared__ __hip_bfloat16 smem[NT_BUF * 2 * BM * BK];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;

  // XCD-contiguous bijective remap over the 1-D grid (8 XCDs)
  int nwg = gridDim.x * gridDim.y;
  int bid = blockIdx.y * gridDim.x + blockIdx.x;
  {
    int q = nwg >> 3, r = nwg & 7, x = bid & 7, o = bid >> 3;
    bid = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + o;
  }
  const int n0 = (bid % gridDim.x) * BN;
  const int m0 = (bid / gridDim.x) * BM;

  // ---- staging: 8 glds per thread per K-tile (4 rounds A + 4 rounds B).
  // Round r covers rows [r*64, r*64+64); within a round, wave w loads rows
  // [w*8, w*8+8), lane: row += lane>>3, 16B chunk = lane&7.  The LDS dest
  // is wave-uniform (glds adds lane*16).
  const int srow = (tid >> 3) & 7;   // row within the wave's 8-row slice
  const int schunk = lane & 7;       // 16B chunk within the 128B row
  auto stage = [&](int buf, int kt) {
    const long long k0 = (long long)kt * BK;
    __hip_bfloat16* sa = smem + buf * (2 * BM * BK);
    __hip_bfloat16* sb = sa + BM * BK;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = r * 64 + wave * 8 + srow;
      const long long kk = k0 + kswz(row, schunk * 16) / 2;
      // LDS base is WAVE-UNIFORM (&s[row0*BK], row0 = r*64+wave*8); the
      // instruction adds lane*16B, which walks exactly rows row0..row0+7
      // (8 lanes per 128B row) because BK*2B == 128B.
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) unsigned int*)(
              A + (long long)(m0 + row) * K + kk),
          (__attribute__((address_space(3))) unsigned int*)(
              sa + (r * 64 + wave * 8) * BK),
          16, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = r * 64 + wave * 8 + srow;
      const long long kk = k0 + kswz(row, schunk * 16) / 2;
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) unsigned int*)(
              B + (long long)(n0 + row) * K + kk),
          (__attribute__((address_space(3))) unsigned int*)(
              sb + (r * 64 + wave * 8) * BK),
          16, 0, 0);
    }
  };

  const int wm = (wave >> 2) * 128;  // wave's M offset in the tile
  const int wn = (wave & 3) * 64;    // wave's N offset

  f32x4 acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // fragment read offsets (bf16 elements from the operand image base):
  // row = frag*16 + (lane&15), kbyte = ks*64 + (lane>>4)*16 (+XOR swizzle)
  const int frow = lane & 15;
  const int fkb = (lane >> 4) * 16;

  const int NT = K / BK;
  stage(0, 0);
  __syncthreads();

  int cur = 0;
  for (int kt = 0; kt < NT; ++kt) {
    if (kt + 1 < NT) stage(cur ^ 1, kt + 1);
    const __hip_bfloat16* sa = smem + cur * (2 * BM * BK);
    const __hip_bfloat16* sb = sa + BM * BK;

    // B fragments for the wave: 4 n-frags x 2 k-steps
    bf16x8 bf[4][2];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const int row = wn + ni * 16 + frow;
        const int kb = kswz(row, ks * 64 + fkb);
        bf[ni][ks] = *(const bf16x8*)((const char*)(sb + row * BK) + kb);
      }
#pragma unroll
    for (int mi = 0; mi < 8; ++mi) {
      bf16x8 af[2];
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const int row = wm + mi * 16 + frow;
        const int kb = kswz(row, ks * 64 + fkb);
        af[ks] = *(const bf16x8*)((const char*)(sa + row * BK) + kb);
      }
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        acc[mi][ni] = mfma16(af[0], bf[ni][0], acc[mi][ni]);
        acc[mi][ni] = mfma16(af[1], bf[ni][1], acc[mi][ni]);
      }
    }
    __syncthreads();
    cur ^= 1;
  }

  // ---- epilogue: stage the C tile (bf16) through LDS for coalesced
  // global rows.  C/D fragment map: col = lane&15, row = (lane>>4)*4+reg.
  float bv[4];
  if (HAS_BIAS) {
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
      bv[ni] = bf2f(bias[n0 + wn + ni * 16 + (lane & 15)]);
  }
  __hip_bfloat16* cs = smem;  // [256][256] bf16 view = 128 KiB
#pragma unroll
  for (int mi = 0; mi < 8; ++mi)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      const int col = wn + ni * 16 + (lane & 15);
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int row = wm + mi * 16 + (lane >> 4) * 4 + reg;
        float v = acc[mi][ni][reg];
        if (HAS_BIAS) v += bv[ni];
        if (RELU) v = fmaxf(v, 0.f);
        cs[row * BN + col] = f2bf(v);
      }
    }
  __syncthreads();
  // 512 threads write 256 rows x 512B: 16 rows per round, 32 chunks/row
  const int wrow = tid >> 5, wchunk = tid & 31;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = r * 16 + wrow;
    *(short8*)((char*)(C + (long long)(m0 + row) * N + n0) + wchunk * 16) =
        *(const short8*)((const char*)(cs + row * BN) + wchunk * 16);
  }
}


// ---------------------------------------------------------------------------
// Split-K variant for TRANSPOSED weight-gradient GEMMs.
//
// dw[N][K] = dy^T @ x is a TN GEMM (both operands M-major) whose transpose
// reads cap the TN kernels near ~450-530 TF.  Transposing BOTH operands
// once (dyT [N][M], xT [K][M] — two HBM passes each over tensors the wgrad
// reads anyway) turns it into THIS kernel: a plain NT GEMM with the huge M
// as the reduction dim — the glds structure's best regime.  The tiny
// output (e.g. 768x2304) parallelizes over grid.z K-chunks; each block
// accumulates its chunk and atomicAdds fp32 fragments into the pre-zeroed
// output (atomics land on a ~few-MB tensor: L2-resident).
__global__ __launch_bounds__(THREADS, 1) void gemm_nt_plain256_splitk_kernel(
    const __hip_bfloat16* __restrict__ A, const __hip_bfloat16* __restrict__ B,
    float* __restrict__ C, int M, int N, int K, int ckt) {
  __shared__ __hip_bfloat16 smem[NT_BUF * 2 * BM * BK];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;

  long long nwg = (long long)gridDim.x * gridDim.y * gridDim.z;
  long long bid = ((long long)blockIdx.z * gridDim.y + blockIdx.y) *
                      gridDim.x + blockIdx.x;
  {
    const long long q = nwg >> 3, r = nwg & 7;
    const int xcd = (int)(bid & 7);
    const long long o = bid >> 3;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + o;
  }
  const int n0 = (int)(bid % gridDim.x) * BN;
  long long t = bid / gridDim.x;
  const int m0 = (int)(t % gridDim.y) * BM;
  const int zi = (int)(t / gridDim.y);
  const int NTt = K / BK;
  const int kt0 = zi * ckt, kt1 = min(NTt, kt0 + ckt);
  if (kt0 >= kt1) return;

  const int srow = (tid >> 3) & 7;
  const int schunk = lane & 7;
  auto stage = [&](int buf, int kt) {
    __hip_bfloat16* sa = smem + buf * (2 * BM * BK);
    __hip_bfloat16* sb = sa + BM * BK;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = r * 64 + wave * 8 + srow;
      const long long kk = (long long)kt * BK + kswz(row, schunk * 16) / 2;
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) unsigned int*)(
              A + (long long)(m0 + row) * M /*lda = reduction dim*/ + kk),
          (__attribute__((address_space(3))) unsigned int*)(
              sa + (r * 64 + wave * 8) * BK),
          16, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = r * 64 + wave * 8 + srow;
      const long long kk = (long long)kt * BK + kswz(row, schunk * 16) / 2;
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) unsigned int*)(
              B + (long long)(n0 + row) * M + kk),
          (__attribute__((address_space(3))) unsigned int*)(
              sb + (r * 64 + wave * 8) * BK),
          16, 0, 0);
    }
  };

  const int wm = (wave >> 2) * 128;
  const int wn = (wave & 3) * 64;
  const int frow = lane & 15;
  const int fkb = (lane >> 4) * 16;

  f32x4 acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  stage(0, kt0);
  __syncthreads();
  int cur = 0;
  for (int kt = kt0; kt < kt1; ++kt) {
    if (kt + 1 < kt1) stage(cur ^ 1, kt + 1);
    const __hip_bfloat16* sa = smem + cur * (2 * BM * BK);
    const __hip_bfloat16* sb = sa + BM * BK;
    bf16x8 bf[4][2];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const int row = wn + ni * 16 + frow;
        bf[ni][ks] = *(const bf16x8*)((const char*)(sb + row * BK) +
                                      kswz(row, ks * 64 + fkb));
      }
#pragma unroll
    for (int mi = 0; mi < 8; ++mi) {
      bf16x8 af[2];
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const int row = wm + mi * 16 + frow;
        af[ks] = *(const bf16x8*)((const char*)(sa + row * BK) +
                                  kswz(row, ks * 64 + fkb));
      }
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        acc[mi][ni] = mfma16(af[0], bf[ni][0], acc[mi][ni]);
        acc[mi][ni] = mfma16(af[1], bf[ni][1], acc[mi][ni]);
      }
    }
    __syncthreads();
    cur ^= 1;
  }

  // fp32 fragment atomics (output is a few MB: L2-resident)
#pragma unroll
  for (int mi = 0; mi < 8; ++mi)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      const int col = n0 + wn + ni * 16 + (lane & 15);
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int row = m0 + wm + mi * 16 + (lane >> 4) * 4 + reg;
        atomicAdd(&C[(long long)row * N + col], acc[mi][ni][reg]);
      }
    }
}

}  // namespace gp

// Host entry: true when the shape is handled (M%256, N%256, K%64, bf16).
bool gemm_nt_plain256(const torch::Tensor& A, const torch::Tensor& B,
                      torch::Tensor& C,
                      const c10::optional<torch::Tensor>& bias, bool relu) {
  static const char* e = getenv("PDT_PLAIN256");
  if (e && e[0] == '0') return false;
  if (A.scalar_type() != torch::kBFloat16) return false;
  const int M = (int)A.size(0), K = (int)A.size(1), N = (int)B.size(0);
  if (M % gp::BM || N % gp::BN || K % gp::BK) return false;
  if (M < 4096) return false;  // small-M shapes: the 128-tile kernel wins
  auto stream = c10::hip::getCurrentHIPStream();
  dim3 grid(N / gp::BN, M / gp::BM);
  const bf16* bias_p = bias.has_value() ? ptr16<bf16>(*bias) : nullptr;
  auto kern = bias_p ? (relu ? &gp::gemm_nt_plain256_kernel<true, true>
                            : &gp::gemm_nt_plain256_kernel<true, false>)
                     : (relu ? &gp::gemm_nt_plain256_kernel<false, true>
                            : &gp::gemm_nt_plain256_kernel<false, false>);
  hipLaunchKernelGGL(kern, grid, dim3(gp::THREADS), 0, stream,
                     ptr16<bf16>(A), ptr16<bf16>(B), ptr16<bf16>(C), bias_p,
                     M, N, K);
  return true;
}

// dw[I][J] (fp32, pre-zeroed by caller semantics: allocated here) from
// TRANSPOSED operands: A=[I][M] (dy^T), B=[J][M] (x^T), both M-contiguous.
torch::Tensor gemm_nt_splitk_f32(torch::Tensor A, torch::Tensor B) {
  TORCH_CHECK(A.dim() == 2 && B.dim() == 2);
  TORCH_CHECK(A.is_contiguous() && B.is_contiguous());
  TORCH_CHECK(A.scalar_type() == torch::kBFloat16 &&
              B.scalar_type() == torch::kBFloat16);
  const int I = (int)A.size(0);
  const long long M = A.size(1);
  const int J = (int)B.size(0);
  TORCH_CHECK(B.size(1) == M, "reduction dim mismatch");
  TORCH_CHECK(I % gp::BM == 0 && J % gp::BN == 0 && M % gp::BK == 0,
              "gemm_nt_splitk_f32 needs I%256, J%256, M%64");
  auto C = torch::zeros({I, J}, A.options().dtype(torch::kFloat32));
  const int NT = (int)(M / gp::BK);
  const int tiles = (I / gp::BM) * (J / gp::BN);
  // target ~1536 blocks (6/CU): enough z to fill the chip on tiny outputs
  int z = std::max(1, std::min(NT, (1536 + tiles - 1) / tiles));
  int ckt = (NT + z - 1) / z;
  z = (NT + ckt - 1) / ckt;
  auto stream = c10::hip::getCurrentHIPStream();
  dim3 grid(J / gp::BN, I / gp::BM, (unsigned)z);
  hipLaunchKernelGGL(gp::gemm_nt_plain256_splitk_kernel, grid,
                     dim3(gp::THREADS), 0, stream,
                     ptr16<bf16>(A), ptr16<bf16>(B), C.data_ptr<float>(), (int)M, J, (int)M, ckt);
  return C;
}
