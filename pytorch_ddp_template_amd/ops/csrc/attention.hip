// Fused multi-head attention FORWARD for gfx950 (CDNA4) — ViT-B/16 shapes.
//
// One workgroup = one (batch n, head h, 32-row q-tile):
//   * stages K and V [S][dh] plus the Q tile straight from the PACKED qkv
//     tensor [N, S, 3, h, dh] via global_load_lds (no q/k/v permute+copy
//     kernels at all),
//   * QK^T on mfma_f32_32x32x16 from LDS,
//   * two-pass row softmax in registers (wave shuffles + one small LDS
//     buffer for the cross-wave max/sum),
//   * writes P (bf16 probabilities) to global — the backward consumes it,
//     exactly like the composed bmm+softmax path saved it,
//   * PV from LDS (P tile written to LDS once), partial sums per wave,
//     LDS-accumulated, written as out[N, S, h*dh] — ready for the proj
//     GEMM, again no permute.
//
// Composed-path equivalence is tested against bmm_nt/softmax/bmm_nn in
// tests/test_gpu_ops.py.  S is runtime (197 for ViT-B/16), padded to a
// multiple of 32 in-kernel; dh must be 64.
#include <torch/extension.h>

#include "common.h"
#include "dispatch.h"

namespace attn {

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
};
template <>
struct MM<_Float16> {
  using vec = f16x8;
  DEV_INLINE static f32x16 mma32(vec a, vec b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
  }
};

constexpr int kDh = 64;        // head dim (fixed)
constexpr int kQT = 32;        // q rows per workgroup
constexpr int kMaxSP = 224;    // padded S capacity (ViT-B/16: S=197)
constexpr int kRow = kDh * 2;  // 128 B per K/V/Q row
// P-tile row stride (elements).  224 would put every row start on the same
// 2 banks (448 B = 112 words, 112 % 32 = 16); 232 gives 8 distinct starts,
// and combined with the chunk swizzle below the PV operand reads are
// conflict-free.
constexpr int kPS = 232;

// K/Q images are 16-B-chunk XOR-swizzled: chunk c of row r is stored at
// chunk position c ^ (r & 7).  Plain row-major 128-B rows put every lane of
// a b128 operand read on the same 4 banks (the row stride is a multiple of
// the 32-bank span -> 32-way conflict, which PMC showed as the kernel being
// wait-bound at 5x SQ_BUSY).  global_load_lds writes lane-linearly, so the
// swizzle is applied to the SOURCE address each lane fetches (the 16-B
// chunks of one 128-B row land permuted but stay in the same cache lines).
// V is NOT swizzled: it is read through ds_read_b64_tr_b16 whose addressing
// is fixed by the transpose unit.
DEV_INLINE int kqswz(int lane8, int row8) { return ((lane8 ^ row8) & 7) * 8; }
// P-tile chunk swizzle (chunks < 28 carry data; chunk 28 is stride pad)
DEV_INLINE int pswz(int row, int col) {
  int c = col >> 3;
  c = c < 28 ? (c ^ (row & 3)) : c;
  return row * kPS + c * 8 + (col & 7);
}

// LDS layout (bytes):
//   K image   [kMaxSP][128]          28672   (chunk-swizzled)
//   V image   [kMaxSP][128]          28672   (natural; tr reads)
//   Q tile    [2][kQT][128]           8192   (chunk-swizzled)
//   P tile    [kQT][kPS*2]           14848   (bf16, swizzled, stride 464 B)
//   red       [2][kQT][4] f32         1024
//   out acc   overlays the P tile (P is dead after PV)
// stats (optional): [2][N*H*S] fp32 — row max of scale*QK^T and 1/rowsum
// (the flash-style backward recomputes P from these instead of reading a
// materialized P).
template <typename T16>
__global__ __launch_bounds__(256, 2) void attn_fwd_kernel(
    const T16* __restrict__ qkv, T16* __restrict__ out, T16* __restrict__ P,
    float* __restrict__ stats, const T16* __restrict__ zpad, int N, int S,
    int H, float scale) {
  __shared__ __attribute__((aligned(16))) char smem[
      kMaxSP * kRow * 2 + 2 * kQT * kRow + kQT * kPS * 2 + 2 * kQT * 4 * 4];
  T16* ldsK = reinterpret_cast<T16*>(smem);
  T16* ldsV = ldsK + kMaxSP * kDh;
  T16* ldsQb = ldsV + kMaxSP * kDh;  // [2][kQT][kDh] double-buffered Q
  T16* ldsP = ldsQb + 2 * kQT * kDh;
  float* red = reinterpret_cast<float*>(ldsP + kQT * kPS);
  // out accumulator overlays the P tile once PV has consumed it
  float* oacc = reinterpret_cast<float*>(ldsP);

  using vec16 = typename MM<T16>::vec;
  const int SP = (S + 31) & ~31;  // padded S actually used
  const int n = blockIdx.z;
  const int hh = blockIdx.y;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int D = H * kDh;
  const long long bh = (long long)n * H + hh;
  const int r32 = lane & 31;
  const int ks = lane >> 5;
  const int nst = SP / 32;  // s-tiles (<= 7)
  const int r8 = lane >> 3;
  const int p16 = (lane & 7) * 8;  // halfword offset within a row

  // ---- stage K and V ONCE for this (n, head): 1 KiB / 8 rows per glds ----
  {
    const int nK = SP / 8;
    for (int u = wave; u < 2 * nK; u += 4) {
      const T16* src = zpad;
      T16* dst;
      int row, which;
      int chunk_off;
      if (u < nK) {
        row = u * 8 + r8; which = 1;
        dst = ldsK + (u * 8) * kDh;
        chunk_off = kqswz(lane, r8);  // K is chunk-swizzled
      } else {
        row = (u - nK) * 8 + r8; which = 2;
        dst = ldsV + ((u - nK) * 8) * kDh;
        chunk_off = p16;  // V natural (tr reads)
      }
      if (row < S)
        src = qkv + (((long long)n * S + row) * 3 + which) * D + hh * kDh +
              chunk_off;
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) unsigned int*)src,
          (__attribute__((address_space(3))) unsigned int*)dst, 16, 0, 0);
    }
  }

  const unsigned tr_off =
      (unsigned)((ks * 8 + ((lane & 15) >> 2)) * (kDh * 2) + (lane & 3) * 8);
  const int img_sel = (lane >> 4) & 1;
#define LDSB(p)                                               \
  ((unsigned)(unsigned long long)(__attribute__((            \
      address_space(3))) const T16*)(p))

  // ---- loop over the q tiles of this (n, head) ----
  // Q is double-buffered: tile t+1's loads are issued before tile t's
  // compute so their latency hides under the MFMAs/softmax.
  auto stage_q = [&](int q0, int buf) {
    for (int u = wave; u < kQT / 8; u += 4) {
      const int row = q0 + u * 8 + r8;
      const T16* src = zpad;
      if (row < S)
        src = qkv + (((long long)n * S + row) * 3 + 0) * D + hh * kDh +
              kqswz(lane, r8);  // Q chunk-swizzled like K
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) unsigned int*)src,
          (__attribute__((address_space(3))) unsigned int*)(
              ldsQb + (buf * kQT + u * 8) * kDh),
          16, 0, 0);
    }
  };
  stage_q(0, 0);
  int qbuf = 0;
  bool first = true;
  for (int q0 = 0; q0 < S; q0 += kQT) {
    const T16* ldsQ = ldsQb + qbuf * kQT * kDh;
    if (q0 + kQT < S) stage_q(q0 + kQT, qbuf ^ 1);
    if (first) {
      __syncthreads();  // drains glds (vmcnt): K/V/Q(0) visible
      first = false;
    }
    // (later barriers in this iteration drain the prefetched Q tile)

    // ---- QK^T (wave w: s-tiles w and w+4) ----
    // chunk index (kc*2+ks) XOR'd with the LDS row's swizzle key; Q
    // fragments hoisted out of the s-tile loop (same row both iterations)
    f32x16 acc[2] = {};
    vec16 aq[4];
#pragma unroll
    for (int kc = 0; kc < 4; ++kc)
      aq[kc] = *reinterpret_cast<const vec16*>(
          ldsQ + r32 * kDh + kqswz(kc * 2 + ks, r32));
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int st = wave + t * 4;
      if (st >= nst) break;
#pragma unroll
      for (int kc = 0; kc < 4; ++kc) {
        vec16 b = *reinterpret_cast<const vec16*>(
            ldsK + (st * 32 + r32) * kDh + kqswz(kc * 2 + ks, r32));
        acc[t] = MM<T16>::mma32(aq[kc], b, acc[t]);
      }
    }

    // ---- row softmax (two passes; regs -> rows (r&3)+8*(r>>2)+4*ks) ----
    float rmax[16], rsum[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float m = -3.0e38f;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int st = wave + t * 4;
        if (st >= nst) break;
        const int col = st * 32 + r32;
        float v = col < S ? acc[t][r] * scale : -3.0e38f;
        m = fmaxf(m, v);
      }
#pragma unroll
      for (int w = 16; w >= 1; w >>= 1) m = fmaxf(m, __shfl_xor(m, w));
      rmax[r] = m;
    }
    if ((lane & 31) == 0) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * ks;
        red[(0 * kQT + row) * 4 + wave] = rmax[r];
      }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = (r & 3) + 8 * (r >> 2) + 4 * ks;
      const float* rw = &red[(0 * kQT + row) * 4];
      rmax[r] = fmaxf(fmaxf(rw[0], rw[1]), fmaxf(rw[2], rw[3]));
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float sm = 0.f;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int st = wave + t * 4;
        if (st >= nst) break;
        const int col = st * 32 + r32;
        float pv = col < S ? __expf(acc[t][r] * scale - rmax[r]) : 0.f;
        acc[t][r] = pv;
        sm += pv;
      }
#pragma unroll
      for (int w = 16; w >= 1; w >>= 1) sm += __shfl_xor(sm, w);
      rsum[r] = sm;
    }
    if ((lane & 31) == 0) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * ks;
        red[(1 * kQT + row) * 4 + wave] = rsum[r];
      }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = (r & 3) + 8 * (r >> 2) + 4 * ks;
      const float* rw = &red[(1 * kQT + row) * 4];
      rsum[r] = 1.f / (rw[0] + rw[1] + rw[2] + rw[3]);
    }

    // ---- softmax stats for the flash backward (once per q row) ----
    if (stats && wave == 0 && r32 == 0) {
      float* sm = stats + bh * S;
      float* sr = stats + ((long long)N * H + bh) * S;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * ks;
        if (q0 + row < S) {
          sm[q0 + row] = rmax[r];
          sr[q0 + row] = rsum[r];
        }
      }
    }

    // ---- P into LDS (the PV operand) ----
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int st = wave + t * 4;
      if (st >= nst) continue;
      const int col = st * 32 + r32;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * ks;
        ldsP[pswz(row, col)] = to_t<T16>(acc[t][r] * rsum[r]);
      }
    }
    for (int c = SP + (int)threadIdx.x; c < kMaxSP; c += 256) {
#pragma unroll
      for (int row = 0; row < kQT; ++row)
        ldsP[pswz(row, c)] = to_t<T16>(0.f);
    }
    __syncthreads();  // ldsP complete

    // ---- bulk-copy P to global from LDS: 16-B stores aligned to the DST
    // (P rows start at (..)*S elements and S is odd for ViT, so row starts
    // are only 2-B aligned: each row gets a scalar head up to the next
    // 16-B boundary, then gathered 16-B chunks; the per-register scatter
    // this replaces was 2-B stores and store-issue-bound).
    // Skipped entirely in flash mode (P == nullptr): the backward
    // recomputes P from the stats, so the S*S materialization disappears
    // from both HBM traffic and activation memory. ----
    if (P) {
      // one row per 8 threads (kQT*8 = 256: no runtime div), units strided 8
      const int spans = (S + 7) / 8 + 1;  // per-row 8-col units (+ head slack)
      const int row = (int)threadIdx.x >> 3;
      if (q0 + row < S) {
        const long long rbase = (bh * S + q0 + row) * (long long)S;
        // head: elements before the first 16-B-aligned dst position
        const int head = (int)((8 - (rbase & 7)) & 7);
        T16* dst = P + rbase;
        for (int unit = (int)threadIdx.x & 7; unit < spans; unit += 8) {
          if (unit == 0) {
            for (int j = 0; j < head && j < S; ++j)
              dst[j] = ldsP[pswz(row, j)];
          } else {
            const int c8 = head + (unit - 1) * 8;
            if (c8 >= S) continue;
            if (c8 + 8 <= S) {
              T16 tmp[8];
#pragma unroll
              for (int j = 0; j < 8; ++j) tmp[j] = ldsP[pswz(row, c8 + j)];
              *reinterpret_cast<uint4*>(dst + c8) =
                  *reinterpret_cast<const uint4*>(tmp);
            } else {
              for (int j = 0; c8 + j < S; ++j)
                dst[c8 + j] = ldsP[pswz(row, c8 + j)];
            }
          }
        }
      }
    }

    // ---- PV: wave-partial over its s-tiles, V^T via hardware tr reads ----
    f32x16 oaccr[2] = {};
    for (int st = wave; st < nst; st += 4) {
#pragma unroll
      for (int kh = 0; kh < 2; ++kh) {
        vec16 a = *reinterpret_cast<const vec16*>(
            ldsP + pswz(r32, st * 32 + kh * 16 + ks * 8));
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          const T16* vimg =
              ldsV + (st * 32 + kh * 16) * kDh + (dt * 32 + img_sel * 16);
          const unsigned b0 = LDSB(vimg) + tr_off;
          v4s l0, h0;
          asm volatile(
              "ds_read_b64_tr_b16 %0, %2 offset:0\n\t"
              "ds_read_b64_tr_b16 %1, %2 offset:512\n\t" /* +4 s-rows */
              "s_waitcnt lgkmcnt(0)"
              : "=&v"(l0), "=&v"(h0)
              : "v"(b0));
          vec16 b;
          reinterpret_cast<v4s*>(&b)[0] = l0;
          reinterpret_cast<v4s*>(&b)[1] = h0;
          oaccr[dt] = MM<T16>::mma32(a, b, oaccr[dt]);
        }
      }
    }
    __syncthreads();  // everyone done reading ldsP; reuse it as oacc
    for (int i = (int)threadIdx.x; i < kQT * kDh; i += 256) oacc[i] = 0.f;
    __syncthreads();
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
      const int col = dt * 32 + r32;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * ks;
        atomicAdd(&oacc[row * kDh + col], oaccr[dt][r]);
      }
    }
    __syncthreads();
    // ---- out[N, S, h*dh]: this head's 128-B slice, 16-B stores ----
    for (int u = wave; u < kQT / 8; u += 4) {
      const int row = u * 8 + r8;
      const int qrow = q0 + row;
      if (qrow >= S) continue;
      T16* dst = out + ((long long)n * S + qrow) * D + hh * kDh + p16;
      const float* srcp = &oacc[row * kDh + p16];
      T16 tmp[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) tmp[j] = to_t<T16>(srcp[j]);
      *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(tmp);
    }
    __syncthreads();  // oacc (= ldsP) read + next Q tile (vmcnt) published
    qbuf ^= 1;
  }
#undef LDSB
}

// tr_off uses a 128-B "row stride" inside the tr pattern; the V image rows
// are kDh*2 = 128 B so the wgrad-style constant folds out — asserted here.
static_assert(kDh * 2 == 128, "tr-read pattern assumes 128-B V rows");

// ===================== flash-style attention BACKWARD =====================
//
// No materialized P and no S×S gradients in HBM: one
// workgroup owns a 64-row K/V tile of one (n, head) and loops over 64-row
// Q tiles, recomputing the P tile from Q/K and the forward's saved softmax
// stats (row max m, 1/rowsum), then chaining five MFMA products per tile
// pair entirely in LDS/registers:
//   S  = Q K^T                 (NT: swizzled Q, swizzled K)
//   P  = exp(scale*S - m) / sum (regs; accumulator layout)
//   dV += P^T dO               (A: tr-read of the P LDS tile; B: tr-read dO)
//   dP = dO V^T                (NT: swizzled dO, swizzled V)
//   dS = P ∘ (dP - D) * scale  (regs; D = rowsum(dO∘O), precomputed)
//   dQ += dS K                 (A: swizzled dS tile;    B: tr-read K)
//   dK += dS^T Q               (A: tr-read of dS tile;  B: tr-read Q)
// dK/dV accumulate in registers across the whole q loop (the block owns
// their rows exclusively) and are written once as bf16.  dQ gets one fp32
// partial per k-tile block ([n_kt][B,S,dh]); the pack kernel reduces the
// (≤4 for ViT) partials while building dqkv — deterministic, no atomics.
//
// Work split: 4 waves = the four 32×32 quadrants of each 64×64 product.
// All LDS images are [64][64] bf16 (128-B rows): natural copies feed the
// hardware transpose reads (ds_read_b64_tr_b16 — fixed 128-B row pattern),
// chunk-XOR-swizzled copies feed the natural b128 operand reads
// (conflict-free, same layout trick as the forward).

constexpr int kBT = 64;  // backward q-tile and k-tile rows

// LDS layout (bf16 units, every image 64*64):
//  Ks Kn Vs | Qs Qn dOs dOn | PSn (P tile, natural; reused for dS) | dSs
// + f32 stats: m[64], r[64], D[64]
constexpr int kImg = kBT * kDh;

template <typename T16>
__global__ __launch_bounds__(256, 2) void attn_bwd_kernel(
    const T16* __restrict__ qkv, const T16* __restrict__ dout,
    const float* __restrict__ stats, const float* __restrict__ Dsum,
    float* __restrict__ dq_partial, T16* __restrict__ dk,
    T16* __restrict__ dv, const T16* __restrict__ zpad, int N, int S, int H,
    float scale) {
  __shared__ __attribute__((aligned(16))) char smem[9 * kImg * 2 + 3 * 64 * 4];
  T16* ldsKs = reinterpret_cast<T16*>(smem);
  T16* ldsKn = ldsKs + kImg;
  T16* ldsVs = ldsKn + kImg;
  T16* ldsQs = ldsVs + kImg;
  T16* ldsQn = ldsQs + kImg;
  T16* ldsOs = ldsQn + kImg;
  T16* ldsOn = ldsOs + kImg;
  T16* ldsPn = ldsOn + kImg;  // P tile (natural); reused as dS natural
  T16* ldsSs = ldsPn + kImg;  // dS tile (swizzled)
  float* stM = reinterpret_cast<float*>(ldsSs + kImg);
  float* stR = stM + 64;
  float* stD = stR + 64;

  using vec16 = typename MM<T16>::vec;
  // XCD-contiguous remap (the k-tile blocks of one (n, head) read the same
  // Q/dO stream — keep them on one XCD's private L2)
  int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
  {
    const int gx = gridDim.x, gy = gridDim.y;
    const long long nwg = (long long)gx * gy * gridDim.z;
    long long id = ((long long)bz * gy + by) * gx + bx;
    if (nwg >= 16) {
      const long long q = nwg >> 3, r = nwg & 7;
      const int xcd = (int)(id & 7);
      const long long idx = id >> 3;
      id = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    bx = (int)(id % gx);
    const long long t = id / gx;
    by = (int)(t % gy);
    bz = (int)(t / gy);
  }
  const int kt = bx;                   // k-tile (64 rows at kt*64)
  const int n = bz;
  const int hh = by;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int D = H * kDh;
  const long long bh = (long long)n * H + hh;
  const long long BS = (long long)N * H * S;
  const int r32 = lane & 31;
  const int ks = lane >> 5;
  const int r8 = lane >> 3;
  const int p16 = (lane & 7) * 8;
  const int k0 = kt * kBT;

  const unsigned tr_off =
      (unsigned)((ks * 8 + ((lane & 15) >> 2)) * (kDh * 2) + (lane & 3) * 8);
  const int img_sel = (lane >> 4) & 1;
#define LDSB(p)                                               \
  ((unsigned)(unsigned long long)(__attribute__((            \
      address_space(3))) const T16*)(p))

  // transposed-operand fragment: IMG^T[c0 + (lane&31)][sum0 + (lane>>5)*8 ..]
  // from a natural [64][64] image (fwd's V-read recipe; valid as A or B —
  // both mfma operand layouts are [l&31][(l>>5)*8+e])
  auto tr_frag = [&](const T16* img, int sum0, int c0) {
    const T16* p = img + sum0 * kDh + (c0 + img_sel * 16);
    const unsigned b0 = LDSB(p) + tr_off;
    v4s l0, h0;
    asm volatile(
        "ds_read_b64_tr_b16 %0, %2 offset:0\n\t"
        "ds_read_b64_tr_b16 %1, %2 offset:512\n\t"
        "s_waitcnt lgkmcnt(0)"
        : "=&v"(l0), "=&v"(h0)
        : "v"(b0));
    vec16 b;
    reinterpret_cast<v4s*>(&b)[0] = l0;
    reinterpret_cast<v4s*>(&b)[1] = h0;
    return b;
  };
  // natural operand fragment from a chunk-swizzled image:
  // IMG[row][kc*16 + ks*8 ..]
  auto sw_frag = [&](const T16* img, int row, int kc) {
    return *reinterpret_cast<const vec16*>(img + row * kDh +
                                           kqswz(kc * 2 + ks, row));
  };

  // ---- stage K (swizzled + natural) and V (swizzled) for this k-tile ----
  {
    for (int u = wave; u < 3 * (kBT / 8); u += 4) {
      const int img = u / (kBT / 8);       // 0=Ks 1=Kn 2=Vs
      const int r0 = (u % (kBT / 8)) * 8;  // 8 rows per unit
      const int row = k0 + r0 + r8;
      const int which = img == 2 ? 2 : 1;  // K or V third of qkv
      const int chunk = img == 1 ? p16 : kqswz(lane, r8);
      const T16* src = zpad;
      if (row < S)
        src = qkv + (((long long)n * S + row) * 3 + which) * D + hh * kDh +
              chunk;
      T16* dst = (img == 0 ? ldsKs : img == 1 ? ldsKn : ldsVs) +
                 (r0 + 0) * kDh;
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) unsigned int*)src,
          (__attribute__((address_space(3))) unsigned int*)dst, 16, 0, 0);
    }
  }

  // persistent per-wave accumulators: quadrant (kq = wave>>1, dq2 = wave&1)
  // of dV and dK [64 k-rows][64 dh]
  f32x16 accV = {};
  f32x16 accK = {};
  const int kq = wave >> 1;   // k-row half for dV/dK outputs
  const int dq2 = wave & 1;   // dh half for dV/dK outputs
  const int qi = wave >> 1;   // q half for S/P/dS/dQ rows
  const int ki = wave & 1;    // k half for S/P/dS cols

  // ---- loop over q tiles ----
  for (int q0 = 0; q0 < S; q0 += kBT) {
    // stage Q (sw+nat), dO (sw+nat), stats/D rows
    __syncthreads();  // previous iteration's readers done
    for (int u = wave; u < 4 * (kBT / 8); u += 4) {
      const int img = u / (kBT / 8);       // 0=Qs 1=Qn 2=dOs 3=dOn
      const int r0 = (u % (kBT / 8)) * 8;
      const int row = q0 + r0 + r8;
      const bool sw = (img & 1) == 0;
      const int chunk = sw ? kqswz(lane, r8) : p16;
      const T16* src = zpad;
      if (row < S) {
        if (img < 2)
          src = qkv + (((long long)n * S + row) * 3 + 0) * D + hh * kDh +
                chunk;
        else
          src = dout + ((long long)n * S + row) * D + hh * kDh + chunk;
      }
      T16* dst =
          (img == 0 ? ldsQs : img == 1 ? ldsQn : img == 2 ? ldsOs : ldsOn) +
          r0 * kDh;
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) unsigned int*)src,
          (__attribute__((address_space(3))) unsigned int*)dst, 16, 0, 0);
    }
    if (threadIdx.x < kBT) {
      const int row = q0 + (int)threadIdx.x;
      const bool ok = row < S;
      stM[threadIdx.x] = ok ? stats[bh * S + row] : 0.f;
      stR[threadIdx.x] = ok ? stats[BS + bh * S + row] : 0.f;
      stD[threadIdx.x] = ok ? Dsum[bh * S + row] : 0.f;
    }
    __syncthreads();  // staging visible (glds drained by the barrier)

    // ---- S quadrant (qi, ki): rows q0+qi*32+., cols k0+ki*32+. ----
    f32x16 accS = {};
#pragma unroll
    for (int kc = 0; kc < 4; ++kc) {
      vec16 a = sw_frag(ldsQs, qi * 32 + r32, kc);
      vec16 b = sw_frag(ldsKs, ki * 32 + r32, kc);
      accS = MM<T16>::mma32(a, b, accS);
    }
    // ---- dP quadrant (qi, ki) = dO V^T ----
    f32x16 accDP = {};
#pragma unroll
    for (int kc = 0; kc < 4; ++kc) {
      vec16 a = sw_frag(ldsOs, qi * 32 + r32, kc);
      vec16 b = sw_frag(ldsVs, ki * 32 + r32, kc);
      accDP = MM<T16>::mma32(a, b, accDP);
    }

    // ---- P and dS in registers; P -> ldsPn (natural) ----
    const int colk = k0 + ki * 32 + r32;   // global k column of this lane
    float pr[16], dsr[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int rowl = qi * 32 + (r & 3) + 8 * (r >> 2) + 4 * ks;
      const float m = stM[rowl];
      const float inv = stR[rowl];  // 0 for padded q rows
      float p = colk < S ? __expf(accS[r] * scale - m) * inv : 0.f;
      pr[r] = p;
      dsr[r] = p * (accDP[r] - stD[rowl]) * scale;
      ldsPn[rowl * kDh + ki * 32 + r32] = to_t<T16>(p);
    }
    __syncthreads();  // ldsPn complete

    // ---- dV += P^T dO : A = tr(Pn) cols kq*32, B = tr(dOn) cols dq2*32 ---
#pragma unroll
    for (int qh = 0; qh < 4; ++qh) {
      vec16 a = tr_frag(ldsPn, qh * 16, kq * 32);
      vec16 b = tr_frag(ldsOn, qh * 16, dq2 * 32);
      accV = MM<T16>::mma32(a, b, accV);
    }
    __syncthreads();  // dV reads done; ldsPn can become dS
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int rowl = qi * 32 + (r & 3) + 8 * (r >> 2) + 4 * ks;
      const T16 v = to_t<T16>(dsr[r]);
      ldsPn[rowl * kDh + ki * 32 + r32] = v;  // natural (tr reads for dK)
      ldsSs[rowl * kDh + kqswz((ki * 32 + r32) >> 3, rowl) +
            ((ki * 32 + r32) & 7)] = v;       // swizzled (A reads for dQ)
    }
    __syncthreads();  // dS tiles complete

    // ---- dQ quadrant (qi, dq2? use (qi, ki) roles: rows q, cols dh) ----
    // wave -> (q half = wave>>1, dh half = wave&1)
    f32x16 accQ = {};
#pragma unroll
    for (int kc = 0; kc < 4; ++kc) {
      vec16 a = sw_frag(ldsSs, qi * 32 + r32, kc);     // dS rows
      vec16 b = tr_frag(ldsKn, kc * 16, dq2 * 32);     // K^T
      accQ = MM<T16>::mma32(a, b, accQ);
    }
    // ---- dK += dS^T Q : A = tr(Pn=dS) cols kq*32, B = tr(Qn) ----
#pragma unroll
    for (int qh = 0; qh < 4; ++qh) {
      vec16 a = tr_frag(ldsPn, qh * 16, kq * 32);
      vec16 b = tr_frag(ldsQn, qh * 16, dq2 * 32);
      accK = MM<T16>::mma32(a, b, accK);
    }

    // ---- write this (q-tile, k-tile) dQ partial (fp32, coalesced) ----
    {
      float* dst = dq_partial + ((long long)kt * N * H + bh) * S * kDh;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rowl = qi * 32 + (r & 3) + 8 * (r >> 2) + 4 * ks;
        const int row = q0 + rowl;
        if (row < S) dst[(long long)row * kDh + dq2 * 32 + r32] = accQ[r];
      }
    }
  }

  // ---- write dK/dV (bf16) — this block owns rows k0..k0+63 exclusively --
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int rowl = kq * 32 + (r & 3) + 8 * (r >> 2) + 4 * ks;
    const int row = k0 + rowl;
    if (row < S) {
      dk[(bh * S + row) * kDh + dq2 * 32 + r32] = to_t<T16>(accK[r]);
      dv[(bh * S + row) * kDh + dq2 * 32 + r32] = to_t<T16>(accV[r]);
    }
  }
#undef LDSB
}

// ===================== flash-style attention FORWARD ======================
//
// The round-1 forward (attn_fwd_kernel above) gives one workgroup a whole
// (n, head) and loops 32-row q-tiles with two-pass softmax: PMC showed it
// wait-bound at 4.3x SQ_BUSY (~45 barriers/block gating ~16 MFMAs each).
// This version is built in the backward kernel's mold — grid over 64-row
// q-tiles (4x the blocks), looping 64-row K/V tiles with ONLINE softmax
// (running row max + rescaled PV accumulator, flash style), ~5 barriers
// per k-tile.  Also removes the S <= 224 cap (K/V are tiled, not staged
// whole) and writes the same stats the flash backward consumes.
// Wave w owns the (w>>1, w&1) 32x32 quadrant of each 64x64 product.
template <typename T16>
__global__ __launch_bounds__(256, 2) void attn_fwd_flash_kernel(
    const T16* __restrict__ qkv, T16* __restrict__ out,
    float* __restrict__ stats, const T16* __restrict__ zpad, int N, int S,
    int H, float scale) {
  __shared__ __attribute__((aligned(16))) char smem[4 * kImg * 2 +
                                                    2 * 128 * 4];
  T16* ldsQs = reinterpret_cast<T16*>(smem);
  T16* ldsKs = ldsQs + kImg;
  T16* ldsVn = ldsKs + kImg;
  T16* ldsPs = ldsVn + kImg;
  float* redM = reinterpret_cast<float*>(ldsPs + kImg);  // [64 rows][2 ki]
  float* redS = redM + 128;                              // [64 rows][2 ki]

  using vec16 = typename MM<T16>::vec;
  // XCD-contiguous remap: the q-tile blocks of one (n, head) read the same
  // K/V; keep them on one XCD's private L2 (x-fastest logical runs).
  int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
  {
    const int gx = gridDim.x, gy = gridDim.y;
    const long long nwg = (long long)gx * gy * gridDim.z;
    long long id = ((long long)bz * gy + by) * gx + bx;
    if (nwg >= 16) {
      const long long q = nwg >> 3, r = nwg & 7;
      const int xcd = (int)(id & 7);
      const long long idx = id >> 3;
      id = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    bx = (int)(id % gx);
    const long long t = id / gx;
    by = (int)(t % gy);
    bz = (int)(t / gy);
  }
  const int q0 = bx * kBT;
  const int n = bz;
  const int hh = by;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int D = H * kDh;
  const long long bh = (long long)n * H + hh;
  const int r32 = lane & 31;
  const int ks = lane >> 5;
  const int r8 = lane >> 3;
  const int p16 = (lane & 7) * 8;
  const int qi = wave >> 1;  // q half (rows)
  const int ki = wave & 1;   // k half for S; dh half for PV

  const unsigned tr_off =
      (unsigned)((ks * 8 + ((lane & 15) >> 2)) * (kDh * 2) + (lane & 3) * 8);
  const int img_sel = (lane >> 4) & 1;
#define LDSB(p)                                               \
  ((unsigned)(unsigned long long)(__attribute__((            \
      address_space(3))) const T16*)(p))
  auto tr_frag = [&](const T16* img, int sum0, int c0) {
    const T16* p = img + sum0 * kDh + (c0 + img_sel * 16);
    const unsigned b0 = LDSB(p) + tr_off;
    v4s l0, h0;
    asm volatile(
        "ds_read_b64_tr_b16 %0, %2 offset:0\n\t"
        "ds_read_b64_tr_b16 %1, %2 offset:512\n\t"
        "s_waitcnt lgkmcnt(0)"
        : "=&v"(l0), "=&v"(h0)
        : "v"(b0));
    vec16 b;
    reinterpret_cast<v4s*>(&b)[0] = l0;
    reinterpret_cast<v4s*>(&b)[1] = h0;
    return b;
  };
  auto sw_frag = [&](const T16* img, int row, int kc) {
    return *reinterpret_cast<const vec16*>(img + row * kDh +
                                           kqswz(kc * 2 + ks, row));
  };

  // ---- stage the Q tile (swizzled) once ----
  for (int u = wave; u < kBT / 8; u += 4) {
    const int row = q0 + u * 8 + r8;
    const T16* src = zpad;
    if (row < S)
      src = qkv + (((long long)n * S + row) * 3 + 0) * D + hh * kDh +
            kqswz(lane, r8);
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) unsigned int*)src,
        (__attribute__((address_space(3))) unsigned int*)(ldsQs + u * 8 * kDh),
        16, 0, 0);
  }

  f32x16 oacc = {};
  float mrow[16], srow[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    mrow[r] = -3.0e38f;
    srow[r] = 0.f;
  }

  const int n_kt = (S + kBT - 1) / kBT;
  for (int kt = 0; kt < n_kt; ++kt) {
    __syncthreads();  // previous iteration's K/V/P readers done
    const int k0 = kt * kBT;
    for (int u = wave; u < 2 * (kBT / 8); u += 4) {
      const int img = u / (kBT / 8);  // 0=Ks 1=Vn
      const int r0 = (u % (kBT / 8)) * 8;
      const int row = k0 + r0 + r8;
      const int which = img == 0 ? 1 : 2;
      const int chunk = img == 0 ? kqswz(lane, r8) : p16;
      const T16* src = zpad;
      if (row < S)
        src = qkv + (((long long)n * S + row) * 3 + which) * D + hh * kDh +
              chunk;
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) unsigned int*)src,
          (__attribute__((address_space(3))) unsigned int*)(
              (img == 0 ? ldsKs : ldsVn) + r0 * kDh),
          16, 0, 0);
    }
    __syncthreads();  // staging visible (barrier drains glds)

    // ---- S quadrant (qi, ki) ----
    f32x16 accS = {};
#pragma unroll
    for (int kc = 0; kc < 4; ++kc) {
      vec16 a = sw_frag(ldsQs, qi * 32 + r32, kc);
      vec16 b = sw_frag(ldsKs, ki * 32 + r32, kc);
      accS = MM<T16>::mma32(a, b, accS);
    }

    // ---- online softmax: per-row tile max within this ki half (32-lane
    // butterfly), cross-ki combine via LDS, exp + tile sums, rescale ----
    const int colk = k0 + ki * 32 + r32;
    const bool colok = colk < S;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float v = colok ? accS[r] * scale : -3.0e38f;
      accS[r] = v;
#pragma unroll
      for (int w = 16; w >= 1; w >>= 1) v = fmaxf(v, __shfl_xor(v, w));
      if (r32 == 0) {
        const int rowl = qi * 32 + (r & 3) + 8 * (r >> 2) + 4 * ks;
        redM[rowl * 2 + ki] = v;
      }
    }
    __syncthreads();  // both ki halves' tile maxes visible
    float alpha[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int rowl = qi * 32 + (r & 3) + 8 * (r >> 2) + 4 * ks;
      const float mnew =
          fmaxf(mrow[r], fmaxf(redM[rowl * 2], redM[rowl * 2 + 1]));
      alpha[r] = mrow[r] == mnew ? 1.f : __expf(mrow[r] - mnew);
      mrow[r] = mnew;
      const float p = colok ? __expf(accS[r] - mnew) : 0.f;
      accS[r] = p;  // now holds this half's P values
      float s = p;
#pragma unroll
      for (int w = 16; w >= 1; w >>= 1) s += __shfl_xor(s, w);
      if (r32 == 0) redS[rowl * 2 + ki] = s;  // this half's TILE sum
      // P tile into LDS (swizzled) for the PV A-operand
      const int c = ki * 32 + r32;
      ldsPs[rowl * kDh + kqswz(c >> 3, rowl) + (c & 7)] = to_t<T16>(p);
    }
    __syncthreads();  // P + both sum halves visible
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int rowl = qi * 32 + (r & 3) + 8 * (r >> 2) + 4 * ks;
      srow[r] = srow[r] * alpha[r] + redS[rowl * 2] + redS[rowl * 2 + 1];
      oacc[r] *= alpha[r];
    }
    // ---- PV quadrant (qi, di = ki): oacc += P · V (unnormalized) ----
#pragma unroll
    for (int kc = 0; kc < 4; ++kc) {
      vec16 a = sw_frag(ldsPs, qi * 32 + r32, kc);
      vec16 b = tr_frag(ldsVn, kc * 16, ki * 32);
      oacc = MM<T16>::mma32(a, b, oacc);
    }
  }

  // ---- finalize: out = oacc / srow, stats = (m, 1/sum) per row ----
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int rowl = qi * 32 + (r & 3) + 8 * (r >> 2) + 4 * ks;
    const int row = q0 + rowl;
    if (row >= S) continue;
    const float inv = 1.f / srow[r];
    out[((long long)n * S + row) * D + hh * kDh + ki * 32 + r32] =
        to_t<T16>(oacc[r] * inv);
    if (ki == 0 && r32 == 0) {
      stats[bh * S + row] = mrow[r];
      stats[((long long)N * H + bh) * S + row] = inv;
    }
  }
#undef LDSB
}

// D = rowsum(dO ∘ O) per (n, head, s) — one wave per (n, s, head) row.
// dout/out are model-layout [N, S, H*dh]; Dsum is [N*H][S] (the backward's
// per-(n,head) indexing).
template <typename T16>
__global__ void attn_bwd_prep_kernel(const T16* __restrict__ dout,
                                     const T16* __restrict__ out,
                                     float* __restrict__ Dsum, int N, int S,
                                     int H) {
  const long long r = (long long)blockIdx.x * 4 + wave_id();  // (n*S+s)*H+hd
  const long long total = (long long)N * S * H;
  if (r >= total) return;
  const long long ns = r / H;  // n*S + s
  const int hd = (int)(r - ns * H);
  const long long n = ns / S;
  const int s = (int)(ns - n * S);
  const int lane = lane_id();
  const T16* a = dout + r * kDh;
  const T16* b = out + r * kDh;
  float acc = to_f(a[lane]) * to_f(b[lane]);
  acc = wave_reduce_sum(acc);
  if (lane == 0) Dsum[(n * H + hd) * (long long)S + s] = acc;
}

// dqkv[n, s, which, hd, :] from: which=0 — sum of n_kt fp32 dq partials;
// which=1/2 — bf16 dk/dv ([N*H, S, dh]).  Same grid/addressing scheme as
// qkv_pack_kernel (16-B units, div-free hot path).
template <typename T16>
__global__ void qkv_pack_flash_kernel(
    const float* __restrict__ dq_partial, const T16* __restrict__ dk,
    const T16* __restrict__ dv, T16* __restrict__ dqkv, int S, int h,
    int n_kt, long long kt_stride, int rcp_h) {
  const int u2 = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (u2 >= 3 * h * (kDh / 8)) return;
  constexpr int lg = 3;  // dh/8 = 8 units (dh = 64)
  const int d8 = u2 & 7;
  const int t = u2 >> lg;                   // which*h + hd
  const int which = (t * rcp_h) >> 16;      // magic /h (t tiny: exact)
  const int hd = t - which * h;
  const int s = (int)blockIdx.y;
  const long long n = blockIdx.z;
  const long long bhs = ((n * h + hd) * (long long)S + s);
  T16 tmp[8];
  if (which == 0) {
    const float* src = dq_partial + bhs * kDh + d8 * 8;
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = src[j];
    for (int kt = 1; kt < n_kt; ++kt) {
      const float* p = src + kt * kt_stride;
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += p[j];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) tmp[j] = to_t<T16>(acc[j]);
  } else {
    const T16* src = (which == 1 ? dk : dv) + bhs * kDh + d8 * 8;
    *reinterpret_cast<uint4*>(tmp) = *reinterpret_cast<const uint4*>(src);
  }
  reinterpret_cast<uint4*>(dqkv)[(((n * S + s) * 3 * h) << lg) + u2] =
      *reinterpret_cast<const uint4*>(tmp);
}

// ---- packed-qkv <-> per-head layout movers for the composed backward ----
// torch's generic 5-D permute+contiguous copies ran at ~140 GB/s and were
// ~6% of the ViT step (89 eager elementwise launches); these are plain
// 16-B-unit copies with both sides coalesced within each dh row.

// All three movers keep per-thread index math to shifts/masks: the big
// non-pow2 dims (n*h, n*S) live on blockIdx.z and are decoded ONCE per
// block with a scalar divide; dh8 must be a pow2 (dh in {8,16,...,128}).
// A first cut decoded a flat index with per-thread 64-bit `/ S` and `% h`
// — it measured SLOWER than torch's generic permute (which uses magic
// dividers); these versions have no per-thread division at all.

// q/k/v[(n*h+hd), s, :] = qkv[n, s, which, hd, :]
// grid: (ceil(S*dh8/256), 3, N*h)
template <typename T16>
__global__ void qkv_unpack_kernel(const T16* __restrict__ qkv,
                                  T16* __restrict__ q, T16* __restrict__ k,
                                  T16* __restrict__ v, int S, int h,
                                  int lg_dh8) {
  const int u2 = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (u2 >= (S << lg_dh8)) return;
  const int s = u2 >> lg_dh8;
  const int d8 = u2 & ((1 << lg_dh8) - 1);
  const int nh = (int)blockIdx.z;           // n*h + hd
  const int n = nh / h, hd = nh - n * h;    // scalar, once per block
  const int which = blockIdx.y;
  T16* outp = which == 0 ? q : which == 1 ? k : v;
  reinterpret_cast<uint4*>(outp)[((long long)nh * S << lg_dh8) + u2] =
      reinterpret_cast<const uint4*>(
          qkv)[((((long long)n * S + s) * 3 + which) * h + hd) << lg_dh8 | d8];
}

// dqkv[n, s, which, hd, :] = {dq,dk,dv}[which][(n*h+hd), s, :]
// grid: (ceil(3*h*dh8/256), S, N)
template <typename T16>
__global__ void qkv_pack_kernel(const T16* __restrict__ dq,
                                const T16* __restrict__ dk,
                                const T16* __restrict__ dv,
                                T16* __restrict__ dqkv, int S, int h,
                                int lg_dh8, int rcp_h) {
  const int u2 = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (u2 >= ((3 * h) << lg_dh8)) return;
  const int d8 = u2 & ((1 << lg_dh8) - 1);
  const int t = u2 >> lg_dh8;               // which*h + hd, < 3*h
  const int which = (t * rcp_h) >> 16;      // magic /h (t tiny: exact)
  const int hd = t - which * h;
  const int s = (int)blockIdx.y;
  const long long n = blockIdx.z;
  const T16* srcp = which == 0 ? dq : which == 1 ? dk : dv;
  reinterpret_cast<uint4*>(
      dqkv)[(((n * S + s) * 3 * h) << lg_dh8) + u2] =
      reinterpret_cast<const uint4*>(
          srcp)[((n * h + hd) * S + s) << lg_dh8 | d8];
}

// y[(n*h+hd), s, :] = x[n, s, hd, :]   (dout head split)
// grid: (ceil(S*dh8/256), 1, N*h)
template <typename T16>
__global__ void head_split_kernel(const T16* __restrict__ x,
                                  T16* __restrict__ y, int S, int h,
                                  int lg_dh8) {
  const int u2 = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (u2 >= (S << lg_dh8)) return;
  const int s = u2 >> lg_dh8;
  const int d8 = u2 & ((1 << lg_dh8) - 1);
  const int nh = (int)blockIdx.z;
  const int n = nh / h, hd = nh - n * h;    // scalar, once per block
  reinterpret_cast<uint4*>(y)[((long long)nh * S << lg_dh8) + u2] =
      reinterpret_cast<const uint4*>(
          x)[(((long long)n * S + s) * h + hd) << lg_dh8 | d8];
}

}  // namespace attn

// out[N,S,H*dh], P[N*H, S, S] (empty when !want_p), stats[2, N*H, S] f32.
// want_p = true materializes P for the composed backward / A-B tests; the
// production path uses want_p = false and the flash backward (attn_bwd).
std::vector<torch::Tensor> attn_fwd(torch::Tensor qkv, int64_t heads,
                                    double scale, bool want_p) {
  TORCH_CHECK(qkv.dim() == 3 && qkv.is_contiguous(),
              "qkv must be [N, S, 3*H*dh] contiguous");
  const int N = (int)qkv.size(0), S = (int)qkv.size(1);
  const int D3 = (int)qkv.size(2);
  const int H = (int)heads;
  TORCH_CHECK(D3 % (3 * H) == 0);
  const int dh = D3 / (3 * H);
  TORCH_CHECK(dh == attn::kDh, "fused attention supports head dim 64");
  // the flash forward tiles K/V (no S cap); only the P-materializing
  // two-pass kernel stages the whole K/V and is capped
  TORCH_CHECK(!want_p || S <= attn::kMaxSP,
              "S too large for the P-materializing kernel");
  auto out = torch::empty({N, S, (long long)H * dh}, qkv.options());
  auto P = want_p
               ? torch::empty({(long long)N * H, S, S}, qkv.options())
               : torch::empty({0}, qkv.options());
  auto stats = torch::empty({2, (long long)N * H, S},
                            qkv.options().dtype(torch::kFloat32));
  static torch::Tensor zp;
  if (!zp.defined() || zp.device() != qkv.device())
    zp = torch::zeros({64}, qkv.options());
  auto stream = c10::hip::getCurrentHIPStream();
  DDP_DISPATCH_FLOAT(qkv.scalar_type(), "attn_fwd", [&] {
    if constexpr (!std::is_same_v<scalar_t, float>) {
      if (!want_p) {
        // flash forward: grid over 64-row q-tiles, online softmax, no P
        dim3 grid((unsigned)((S + attn::kBT - 1) / attn::kBT), H, N);
        hipLaunchKernelGGL((attn::attn_fwd_flash_kernel<scalar_t>), grid,
                           dim3(256), 0, stream,
                           reinterpret_cast<const scalar_t*>(qkv.data_ptr()),
                           reinterpret_cast<scalar_t*>(out.data_ptr()),
                           stats.data_ptr<float>(),
                           reinterpret_cast<const scalar_t*>(zp.data_ptr()),
                           N, S, H, (float)scale);
      } else {
        dim3 grid(1, H, N);  // q-tiles looped in-kernel (K/V staged once)
        hipLaunchKernelGGL((attn::attn_fwd_kernel<scalar_t>), grid, dim3(256),
                           0, stream,
                           reinterpret_cast<const scalar_t*>(qkv.data_ptr()),
                           reinterpret_cast<scalar_t*>(out.data_ptr()),
                           reinterpret_cast<scalar_t*>(P.data_ptr()),
                           stats.data_ptr<float>(),
                           reinterpret_cast<const scalar_t*>(zp.data_ptr()),
                           N, S, H, (float)scale);
      }
    } else {
      TORCH_CHECK(false, "attn_fwd: bf16/f16 only");
    }
  });
  return {out, P, stats};
}

// Flash-style fused backward: dqkv from (qkv, dout, out, stats).  No S×S
// tensors touch HBM; see attn_bwd_kernel.
torch::Tensor attn_bwd(torch::Tensor qkv, torch::Tensor dout,
                       torch::Tensor out, torch::Tensor stats, int64_t heads,
                       double scale) {
  TORCH_CHECK(qkv.dim() == 3 && qkv.is_contiguous());
  TORCH_CHECK(dout.is_contiguous() && out.is_contiguous());
  const int N = (int)qkv.size(0), S = (int)qkv.size(1);
  const int H = (int)heads;
  const int dh = (int)(qkv.size(2) / (3 * H));
  TORCH_CHECK(dh == attn::kDh, "flash backward supports head dim 64");
  TORCH_CHECK(stats.scalar_type() == torch::kFloat32 &&
              stats.numel() == 2LL * N * H * S);
  TORCH_CHECK(H <= 128, "qkv_pack_flash magic-reciprocal bound");
  const int n_kt = (S + attn::kBT - 1) / attn::kBT;
  const long long B = (long long)N * H;
  auto f32 = qkv.options().dtype(torch::kFloat32);
  auto Dsum = torch::empty({B, S}, f32);
  auto dq_partial = torch::empty({n_kt, B, (long long)S, attn::kDh}, f32);
  auto dk = torch::empty({B, (long long)S, attn::kDh}, qkv.options());
  auto dv = torch::empty({B, (long long)S, attn::kDh}, qkv.options());
  auto dqkv = torch::empty_like(qkv);
  static torch::Tensor zp;
  if (!zp.defined() || zp.device() != qkv.device())
    zp = torch::zeros({64}, qkv.options());
  auto stream = c10::hip::getCurrentHIPStream();
  TORCH_CHECK(N <= 65535 && S <= 65535 && n_kt <= 65535);
  DDP_DISPATCH_FLOAT(qkv.scalar_type(), "attn_bwd", [&] {
    if constexpr (!std::is_same_v<scalar_t, float>) {
      const long long rows = (long long)N * S * H;
      hipLaunchKernelGGL((attn::attn_bwd_prep_kernel<scalar_t>),
                         dim3((unsigned)((rows + 3) / 4)), dim3(256), 0,
                         stream,
                         reinterpret_cast<const scalar_t*>(dout.data_ptr()),
                         reinterpret_cast<const scalar_t*>(out.data_ptr()),
                         Dsum.data_ptr<float>(), N, S, H);
      hipLaunchKernelGGL((attn::attn_bwd_kernel<scalar_t>),
                         dim3(n_kt, H, N), dim3(256), 0, stream,
                         reinterpret_cast<const scalar_t*>(qkv.data_ptr()),
                         reinterpret_cast<const scalar_t*>(dout.data_ptr()),
                         stats.data_ptr<float>(), Dsum.data_ptr<float>(),
                         dq_partial.data_ptr<float>(),
                         reinterpret_cast<scalar_t*>(dk.data_ptr()),
                         reinterpret_cast<scalar_t*>(dv.data_ptr()),
                         reinterpret_cast<const scalar_t*>(zp.data_ptr()), N,
                         S, H, (float)scale);
      dim3 pgrid((unsigned)((3 * H * (attn::kDh / 8) + 255) / 256),
                 (unsigned)S, (unsigned)N);
      hipLaunchKernelGGL((attn::qkv_pack_flash_kernel<scalar_t>), pgrid,
                         dim3(256), 0, stream, dq_partial.data_ptr<float>(),
                         reinterpret_cast<const scalar_t*>(dk.data_ptr()),
                         reinterpret_cast<const scalar_t*>(dv.data_ptr()),
                         reinterpret_cast<scalar_t*>(dqkv.data_ptr()), S, H,
                         n_kt, B * (long long)S * attn::kDh, 65536 / H + 1);
    } else {
      TORCH_CHECK(false, "attn_bwd: bf16/f16 only");
    }
  });
  return dqkv;
}

// qkv [N, S, 3*h*dh] -> (q, k, v) each [N*h, S, dh]
std::vector<torch::Tensor> qkv_unpack(torch::Tensor qkv, int64_t heads) {
  TORCH_CHECK(qkv.dim() == 3 && qkv.is_contiguous());
  const int N = (int)qkv.size(0), S = (int)qkv.size(1);
  const int h = (int)heads;
  const int dh = (int)(qkv.size(2) / (3 * h));
  const int lg = log2_exact(dh / 8);
  TORCH_CHECK(dh % 8 == 0 && lg >= 0, "qkv_unpack needs pow2 dh/8");
  auto opt = qkv.options();
  auto q = torch::empty({(long long)N * h, S, dh}, opt);
  auto k = torch::empty({(long long)N * h, S, dh}, opt);
  auto v = torch::empty({(long long)N * h, S, dh}, opt);
  TORCH_CHECK((long long)N * h <= 65535, "qkv_unpack grid.z limit");
  dim3 grid((unsigned)(((S << lg) + 255) / 256), 3, (unsigned)(N * h));
  auto stream = c10::hip::getCurrentHIPStream();
  DDP_DISPATCH_FLOAT(qkv.scalar_type(), "qkv_unpack", [&] {
    if constexpr (!std::is_same_v<scalar_t, float>) {
      hipLaunchKernelGGL((attn::qkv_unpack_kernel<scalar_t>), grid, dim3(256),
                         0, stream,
                         reinterpret_cast<const scalar_t*>(qkv.data_ptr()),
                         reinterpret_cast<scalar_t*>(q.data_ptr()),
                         reinterpret_cast<scalar_t*>(k.data_ptr()),
                         reinterpret_cast<scalar_t*>(v.data_ptr()), S, h, lg);
    } else {
      TORCH_CHECK(false, "qkv_unpack: bf16/f16 only");
    }
  });
  return {q, k, v};
}

// (dq, dk, dv) each [N*h, S, dh] -> dqkv [N, S, 3*h*dh]
torch::Tensor qkv_pack(torch::Tensor dq, torch::Tensor dk, torch::Tensor dv,
                       int64_t N, int64_t heads) {
  TORCH_CHECK(dq.is_contiguous() && dk.is_contiguous() && dv.is_contiguous());
  TORCH_CHECK(dq.scalar_type() == dk.scalar_type() &&
              dq.scalar_type() == dv.scalar_type());
  const int h = (int)heads;
  const int S = (int)dq.size(1), dh = (int)dq.size(2);
  const int lg = log2_exact(dh / 8);
  TORCH_CHECK(dh % 8 == 0 && lg >= 0, "qkv_pack needs pow2 dh/8");
  auto dqkv = torch::empty({N, S, (long long)3 * h * dh}, dq.options());
  TORCH_CHECK(N <= 65535 && S <= 65535, "qkv_pack grid limits");
  // The kernel decodes which/hd with the magic reciprocal 65536/h + 1, exact
  // only while (3h-1)*(65536/h + 1) < 65536*(t/h + 1) — holds for h <= 128;
  // larger head counts would silently mis-route gradients.
  TORCH_CHECK(h >= 1 && h <= 128, "qkv_pack: heads must be in [1,128], got ",
              h);
  dim3 grid((unsigned)((((3 * h) << lg) + 255) / 256), (unsigned)S,
            (unsigned)N);
  auto stream = c10::hip::getCurrentHIPStream();
  DDP_DISPATCH_FLOAT(dq.scalar_type(), "qkv_pack", [&] {
    if constexpr (!std::is_same_v<scalar_t, float>) {
      hipLaunchKernelGGL((attn::qkv_pack_kernel<scalar_t>), grid, dim3(256),
                         0, stream,
                         reinterpret_cast<const scalar_t*>(dq.data_ptr()),
                         reinterpret_cast<const scalar_t*>(dk.data_ptr()),
                         reinterpret_cast<const scalar_t*>(dv.data_ptr()),
                         reinterpret_cast<scalar_t*>(dqkv.data_ptr()), S, h,
                         lg, 65536 / h + 1);
    } else {
      TORCH_CHECK(false, "qkv_pack: bf16/f16 only");
    }
  });
  return dqkv;
}

// x [N, S, h*dh] -> y [N*h, S, dh]
torch::Tensor head_split(torch::Tensor x, int64_t heads) {
  TORCH_CHECK(x.dim() == 3 && x.is_contiguous());
  const int N = (int)x.size(0), S = (int)x.size(1);
  const int h = (int)heads;
  const int dh = (int)(x.size(2) / h);
  const int lg = log2_exact(dh / 8);
  TORCH_CHECK(dh % 8 == 0 && lg >= 0, "head_split needs pow2 dh/8");
  auto y = torch::empty({(long long)N * h, S, dh}, x.options());
  TORCH_CHECK((long long)N * h <= 65535, "head_split grid.z limit");
  dim3 grid((unsigned)(((S << lg) + 255) / 256), 1, (unsigned)(N * h));
  auto stream = c10::hip::getCurrentHIPStream();
  DDP_DISPATCH_FLOAT(x.scalar_type(), "head_split", [&] {
    if constexpr (!std::is_same_v<scalar_t, float>) {
      hipLaunchKernelGGL((attn::head_split_kernel<scalar_t>), grid, dim3(256),
                         0, stream,
                         reinterpret_cast<const scalar_t*>(x.data_ptr()),
                         reinterpret_cast<scalar_t*>(y.data_ptr()), S, h, lg);
    } else {
      TORCH_CHECK(false, "head_split: bf16/f16 only");
    }
  });
  return y;
}
