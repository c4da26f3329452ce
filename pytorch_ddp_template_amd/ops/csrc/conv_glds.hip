// Implicit-GEMM conv forward on the glds 256-tile structure (gfx950).
//
// y[M][Kout] = im2col(x)[M][RSC] @ w[Kout][RSC]^T  (NHWC, weight (K,R,S,C))
// — the weight tensor IS a contiguous [Kout][R*S*C] NT operand, and with
// C % 64 == 0 every 64-deep K-tile lives inside ONE tap (r,s), so the
// A-side im2col gather is a single per-row base + 16B chunk: exactly the
// glds staging pattern of gemm_plain.hip, with the gather folded into the
// per-lane SOURCE address (glds destinations stay lane-linear).
//
// Same structure as gemm_nt_plain256 (measured ~2x the older NT conv
// kernels' TF on plain shapes): BK=64, two LDS buffers, one barrier per
// K-tile with the next tile's glds issued before the MFMAs, source-side
// XOR k-slot swizzle, mfma_f32_16x16x32_bf16, XCD-bijective remap,
// LDS-staged coalesced epilogue.  Optional BN-stats epilogue (partial
// col sums/sumsq) matching the NT/halo workspace convention so the fused
// conv+BN path (bn_fwd_ws) consumes it unchanged.  Optional dgrad epilogue
// (skip-grad addend and/or ReLU mask in the coalesced store phase, EPI_*).
// With EPI_BNSTATS the masked dgrad also leaves the per-channel BatchNorm
// backward sums (sum dz, sum dz*xhat) of the BN it feeds in a workspace that
// bn_bwd_finalize_kernel consumes, so that BN's stats pass disappears
// (bn_bwd_ws) — the backward mirror of the forward stats epilogue.
//
// Eligibility (host): bf16, pow2 C >= 64, M % 256 == 0, Kout % 64 == 0.
// Tiles: BM=256 by BN=256/128/64 (by Kout) — always 8 waves as 2(M)x4(N),
// per-wave 128 M-rows (MI=8), NI = BN/64.  BN=64 tiles are 80 KB of LDS and
// run two blocks per CU (better glds latency hiding).
// Covers every non-stem ResNet-18/CIFAR conv (fwd and, via the rotated-
// weight identity, stride-1 dgrad).  Reference scope: SURVEY §2b conv row.
//
// Halo-resident A (template parameter HW; the 64-wide tile, and the 128-wide
// tile at HW = 16): the per-tap
// gather above re-reads every input element once per tap, and the engine is
// bound by that cache-to-LDS fill, not by MFMA or HBM (profiles/
// r06_conv_halo64.md).  For 3x3 stride-1 pad-1 convs with C = 64 whose M-tile
// is whole rows of one image (W = 16, 32 or 64; conv_halo64_eligible) the
// block stages its (256/W + 2) x (W + 2) input patch once, and the K-loop
// streams only the 8-KB weight tile of each tap; same K order, same MFMA
// sequence per output element, every epilogue shared, so results are
// bit-identical to the per-tap route.  PDT_CONV_HALO64=0 (read per call)
// restores the per-tap route for A/B runs.  The 128-wide tile does the same
// for C = 128 on 16-wide images (conv_halo128_eligible, PDT_CONV_HALO128=0;
// profiles/r09_conv_halo128.md): the 18 x 18 patch is two 64-channel planes
// and the K-loop streams the 16-KB weight tile of each (tap, channel slice).
//
// Parity-split stride-2 dgrad (template parameter PAR, all three tile widths,
// the five dgrad epilogue modes): a 3x3 stride-2 pad-1 dgrad run as a stride-1
// conv over the zero-stuffed dy executes nine taps per dx pixel of which only
// 1, 2, 2 or 4 (by pixel parity) carry data.  With PAR an M-tile holds pixels
// of one parity class and the K-loop runs that class's taps only: a quarter of
// the fills, LDS reads and MFMAs, same products in the same order, shared
// epilogues with the row address mapped to (n, 2i + a, 2j + b); dx is
// bit-identical to the stuffed route (profiles/r07_dgrad_s2_parity.md).
// conv_dgrad_s2_parity_eligible is the gate; PDT_DGRAD_S2_PARITY=0 (read per
// call) restores the stuffed route for A/B runs.

#include <torch/extension.h>

#include "common.h"
#include "dispatch.h"

namespace cg {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int BM = 256, BK = 64;
constexpr int THREADS = 512;

__device__ __forceinline__ f32x4 mfma16(bf16x8 a, bf16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ int kswz(int row, int kbyte) {
  return kbyte ^ (((row >> 2) & 1) << 5);
}

struct Geom {
  int H, W, C, lgC, HO, WO, stride, pad, S, RS;  // S = kernel width
  // transposed-conv (stride-s dgrad) gather: the logical image is the
  // zero-STUFFED dy — coordinates valid only on the stride grid, source
  // indexed by the un-stuffed position.  lgSt=0 -> plain conv (H,W = real
  // source dims).
  int lgSt = 0;
};

// Store-phase epilogue modes (dgrad only; bit 0 = addend, bit 1 = mask):
//   y = relu_bwd(bf16(float(bf16(acc)) + float(addend)), out_mask)
// with each part optional.  Both operands are read in the coalesced store
// layout (one 16-B chunk per lane per row), AFTER the accumulator has been
// rounded to bf16 — bit-identical to the separate ew::AddOp / ew::ReluBwdOp
// passes it replaces.
constexpr int EPI_NONE = 0, EPI_ADD = 1, EPI_MASK = 2, EPI_ADD_MASK = 3;
// bit 2 = BN-backward sums of the stored (masked) values; only together with
// the mask and without an addend.  The addend operand slot then carries the
// BN input t, and for every stored element v (column c)
//   ws[R + row][c] += v          ws[row][c] += v * (t - mean[c]) * rstd[c]
// with row = block id % R: the [2R][C] layout of bn_bwd_stats_kernel.
constexpr int EPI_BNSTATS = 4, EPI_MASK_BNSTATS = EPI_MASK | EPI_BNSTATS;

// Halo-resident A operand (HW != 0; 64-wide tile, 3x3 stride-1 pad-1, C = 64,
// image width HW): a 256-row M-tile is BM/HW whole rows of one image, so its
// input patch — those rows plus one above, one below and a column each side —
// is staged ONCE and all nine taps read it, instead of re-gathering the tile
// per tap.  Halo rows are HP positions apart (HW + 2 rounded up to 8); a
// 1-KiB piece is 8 positions stored chunk-major, [16-B chunk][position & 7],
// by swapping the roles of lane>>3 and lane&7 in the glds SOURCE address.
// The 16 rows of an A fragment are 16 consecutive positions, so every
// ds_read_b128 lane group covers 8 consecutive positions of an even chunk and
// 8 of an odd one: all 16 slots of the 256-B bank row, conflict-free for any
// tap shift.  A tap (r, s) is then the per-lane address of column shift s
// plus the constant (r * HP + ...) * 128 — no address arithmetic in the loop.
//
// 128-wide tile (BN = 128, HW = 16, C = 128): BN / 64 = 2 such planes, plane p
// holding channels 64p .. 64p + 63 in exactly the layout above and starting
// at p * halo_bytes(16) = p * 55,296 B.  That offset is a multiple of 1 KiB,
// so a plane-1 read hits the banks of the same read in plane 0 and the
// conflict-free enumeration above carries over unchanged.  K stays tap-major,
// then the two 64-channel slices (kt = tap * 2 + slice), so a step adds its
// slice's plane offset to the tap's address and streams weight tile kt.
// 110,592 B of patch + 2 x 16 KB of weight buffers = 143,360 B: one block per
// CU, as on the per-tap 128-wide tile.
constexpr int halo_pitch(int hw) { return (hw + 2 + 7) & ~7; }
constexpr int halo_bytes(int hw) {
  return hw ? (BM / hw + 2) * halo_pitch(hw) * BK * 2 : 0;
}

// Parity-split stride-2 dgrad (PAR; 3x3 stride-2 pad-1, dy dims H x W powers
// of two, dx = 2H x 2W): the stuffed gather above runs all nine taps over every
// dx pixel although a pixel of parity class (a, b) = (h & 1, w & 1) has only
// (1 + a) * (1 + b) taps on the stride grid.  Here an M-tile is 256
// consecutive dy positions (n, i, j) of ONE class, its rows are the dx pixels
// (n, 2i + a, 2j + b), and the K-loop runs the class's taps only.  With the
// rotated weight and dpad = 1 the stuffed source row of tap rt is h - 1 + rt:
//   even h = 2i     : rt = 1 only             -> dy row i
//   odd  h = 2i + 1 : rt = 0 -> dy row i,  rt = 2 -> dy row i + 1
// and the same for columns (st, j).  A source index equal to H or W (the last
// odd row / column) reads the zero page.  Taps run in ascending (rt, st)
// order with today's weight tile addresses, so every dx element sums the same
// nonzero products in the same order as on the stuffed route, which only adds
// exact zeros in between.  The class is the low two bits of the remapped tile
// index, so every XCD gets the same mix of 1-, 2- and 4-tap tiles and the
// four classes of one position tile read the same dy rows through one L2.
//
// (the second launch bound is waves per SIMD: the 64-wide halo variant asks
// for the 4 that two co-resident blocks need, i.e. at most 128 VGPRs; the
// 128-wide one runs one block per CU)
template <int BN, bool STATS, int EPI = EPI_NONE, int HW = 0, bool PAR = false>
__global__ __launch_bounds__(THREADS,
                             HW ? (BN == 64 ? 4 : 1) : BN == 64 ? 2 : 1)
void conv_fwd_glds_kernel(
    const __hip_bfloat16* __restrict__ x, const __hip_bfloat16* __restrict__ w,
    __hip_bfloat16* __restrict__ y, const __hip_bfloat16* __restrict__ zpad,
    int M, int N /*Kout*/, int K /*RSC*/, Geom g,
    float* __restrict__ stats_ws, int ws_nblocks,
    const __hip_bfloat16* __restrict__ addend,
    const __hip_bfloat16* __restrict__ out_mask,
    const float* __restrict__ bn_mean, const float* __restrict__ bn_rstd) {
  static_assert(!(STATS && EPI != EPI_NONE),
                "dgrad epilogues carry no forward stats");
  static_assert(!(EPI & EPI_BNSTATS) || EPI == EPI_MASK_BNSTATS,
                "BN-backward sums ride only with the mask, without an addend");
  static_assert(HW == 0 || ((BN == 64 || (BN == 128 && HW == 16)) &&
                            BM % HW == 0 && HW % 16 == 0),
                "halo variant: 64-wide tile, or 128-wide at HW = 16; whole "
                "image rows per M-tile");
  static_assert(!PAR || (!STATS && HW == 0),
                "parity split: dgrad only, per-tap gather");
  constexpr int HALO_ELEMS = halo_bytes(HW) / 2;  // one 64-channel plane
  constexpr int NPL = HW ? BN / 64 : 0;           // planes (host: C == BN)
  __shared__ __hip_bfloat16
      smem[HW ? NPL * HALO_ELEMS + 2 * BN * BK : 2 * (BM + BN) * BK];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;

  long long nwg = (long long)gridDim.x * gridDim.y;
  long long bid = (long long)blockIdx.y * gridDim.x + blockIdx.x;
  {
    const long long q = nwg >> 3, r = nwg & 7;
    const int xcd = (int)(bid & 7);
    const long long o = bid >> 3;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + o;
  }
  const int n0 = (int)(bid % gridDim.x) * BN;
  const long long mtile = bid / gridDim.x;
  // PAR: class (pa, pb) = (h & 1, w & 1) of the tile's dx pixels; m0 then
  // counts dy positions
  const int pa = PAR ? (int)(mtile >> 1) & 1 : 0;
  const int pb = PAR ? (int)mtile & 1 : 0;
  const long long m0 = (PAR ? mtile >> 2 : mtile) * BM;
  const int lgH = PAR ? 31 - __clz(g.H) : 0, lgW = PAR ? 31 - __clz(g.W) : 0;
  const long long flat_id = bid;

  // ---- staging geometry (v1 pattern): per round 64 rows; wave w rows
  // [w*8, +8), lane: row += lane>>3, chunk = lane&7.
  const int srow = (tid >> 3) & 7;
  const int schunk = lane & 7;
  constexpr int RA = BM / 64;  // A rounds per K-tile
  constexpr int RB = BN / 64;  // B rounds

  // Per-row gather bases hoisted out of the K-loop: this thread stages the
  // same M-rows every tile.  hi/wi validity is per-tap, so keep the
  // unshifted coordinates.
  long long nbase[RA];
  int hv[RA], wv[RA];
#pragma unroll
  for (int r = 0; r < RA; ++r) {
    // hoisted out of the K-loop, so plain div/mod (non-pow2 spatial: the
    // ResNet-50 224-input pyramid is 56/28/14/7) costs nothing hot
    const long long m = m0 + r * 64 + wave * 8 + srow;
    if constexpr (PAR) {
      // pow2 dy dims: m IS the dy position of tap offset (0, 0)
      hv[r] = (int)(m >> lgW) & (g.H - 1);
      wv[r] = (int)m & (g.W - 1);
      nbase[r] = m;
      continue;
    }
    const int wo = (int)(m % g.WO);
    const long long t = m / g.WO;
    const int ho = (int)(t % g.HO);
    const long long n = t / g.HO;
    hv[r] = ho * g.stride - g.pad;
    wv[r] = wo * g.stride - g.pad;
    nbase[r] = n * g.H * (long long)g.W;
  }
  const int smask = (1 << g.lgSt) - 1;

  auto stage = [&](int buf, int kt) {
    __hip_bfloat16* sa = smem + buf * ((BM + BN) * BK);
    __hip_bfloat16* sb = sa + BM * BK;
    int tap = (kt << 6) >> g.lgC;
    const int c0 = (kt << 6) & (g.C - 1);
    // PAR: kt counts the class's taps only; its tap index is (dh, dw) in
    // {0, 1}^2, the source offset, and (rt, st) = (pa ? 2 dh : 1, pb ? 2 dw : 1)
    const int dh = pb ? tap >> 1 : tap, dw = pb ? tap & 1 : 0;
    int wkt = kt;  // k-tile of the weight operand
    if constexpr (PAR) {
      tap = (pa ? 2 * dh : 1) * 3 + (pb ? 2 * dw : 1);
      wkt = (tap << (g.lgC - 6)) + (c0 >> 6);
    }
    const int rt = tap / g.S, st = tap - rt * g.S;
#pragma unroll
    for (int r = 0; r < RA; ++r) {
      const int row = r * 64 + wave * 8 + srow;
      const int kk = c0 + kswz(row, schunk * 16) / 2;
      const __hip_bfloat16* src = zpad;
      const int hs = hv[r] + rt, ws = wv[r] + st;
      if constexpr (PAR) {
        if (hv[r] + dh < g.H && wv[r] + dw < g.W)
          src = x + ((nbase[r] + dh * g.W + dw) << g.lgC) + kk;
      } else if ((unsigned)(hs >> g.lgSt) < (unsigned)g.H &&
          (unsigned)(ws >> g.lgSt) < (unsigned)g.W &&
          ((hs | ws) & smask) == 0)
        src = x + ((nbase[r] + (long long)(hs >> g.lgSt) * g.W +
                    (ws >> g.lgSt))
                   << g.lgC) +
              kk;
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) unsigned int*)src,
          (__attribute__((address_space(3))) unsigned int*)(
              sa + (r * 64 + wave * 8) * BK),
          16, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < RB; ++r) {
      const int row = r * 64 + wave * 8 + srow;
      const long long kk = (long long)wkt * BK + kswz(row, schunk * 16) / 2;
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) unsigned int*)(
              w + (long long)(n0 + row) * K + kk),
          (__attribute__((address_space(3))) unsigned int*)(
              sb + (r * 64 + wave * 8) * BK),
          16, 0, 0);
    }
  };

  // wave grid: always 128 M-rows per wave (MI=8)
  constexpr int NWM = BM / 128;          // waves along M
  constexpr int NWN = 8 / NWM;           // waves along N
  constexpr int NI = BN / (16 * NWN);    // 16-col frags per wave (4, 2 or 1)
  const int wm = (wave / NWN) * 128;
  const int wn = (wave % NWN) * (NI * 16);
  const int frow = lane & 15;
  const int fkb = (lane >> 4) * 16;

  f32x4 acc[8][NI];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  if constexpr (HW == 0) {
    const int NT = PAR ? ((1 + pa) * (1 + pb)) << (g.lgC - 6) : K / BK;
    stage(0, 0);
    __syncthreads();

    int cur = 0;
    for (int kt = 0; kt < NT; ++kt) {
      if (kt + 1 < NT) stage(cur ^ 1, kt + 1);
      const __hip_bfloat16* sa = smem + cur * ((BM + BN) * BK);
      const __hip_bfloat16* sb = sa + BM * BK;
      bf16x8 bf[NI][2];
#pragma unroll
      for (int ni = 0; ni < NI; ++ni)
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
        for (int ni = 0; ni < NI; ++ni) {
          acc[mi][ni] = mfma16(af[0], bf[ni][0], acc[mi][ni]);
          acc[mi][ni] = mfma16(af[1], bf[ni][1], acc[mi][ni]);
        }
      }
      __syncthreads();
      cur ^= 1;
    }
  } else {
    // ---- halo-resident A: stage the patch once, stream only the weights
    constexpr int HP = halo_pitch(HW);
    constexpr int KR = BM / HW;                 // image rows per M-tile
    constexpr int PPR = HP / 8;                 // 1-KiB pieces per halo row
    constexpr int PLPIECE = (KR + 2) * PPR;     // pieces per plane
    constexpr int NPIECE = NPL * PLPIECE;
    constexpr int LGCH = BN == 64 ? 6 : 7;      // log2 C: the position stride
    __hip_bfloat16* sw = smem + NPL * HALO_ELEMS;  // two weight tiles
    const int tpi = g.H / KR;                   // M-tiles per image
    const int tile = (int)(m0 / BM);            // host: M / BM fits an int
    const long long img = tile / tpi;
    const int h0 = (tile - (int)img * tpi) * KR;

    auto stage_w = [&](int buf, int kt) {
      __hip_bfloat16* sb = sw + buf * (BN * BK);
#pragma unroll
      for (int r = 0; r < RB; ++r) {
        const int row = r * 64 + wave * 8 + srow;
        const long long kk = (long long)kt * BK + kswz(row, schunk * 16) / 2;
        __builtin_amdgcn_global_load_lds(
            (const __attribute__((address_space(1))) unsigned int*)(
                w + (long long)(n0 + row) * K + kk),
            (__attribute__((address_space(3))) unsigned int*)(
                sb + (r * 64 + wave * 8) * BK),
            16, 0, 0);
      }
    };
    stage_w(0, 0);
    // piece pc = 8 positions of halo row pc / PPR (of plane pc / PLPIECE, the
    // planes being PLPIECE KiB apart); lane: position lane & 7, chunk
    // lane >> 3.  Rows outside the image, the two border columns and the
    // pitch padding come from the zero page.
#pragma unroll
    for (int p0 = 0; p0 < NPIECE; p0 += 8) {
      const int pc = p0 + wave;
      if (pc < NPIECE) {
        const int pl = NPL > 1 ? pc / PLPIECE : 0;
        const int pp = pc - pl * PLPIECE;
        const int hr = pp / PPR;
        const int hi = h0 - 1 + hr;
        const int wi = (pp - hr * PPR) * 8 + (lane & 7) - 1;
        const __hip_bfloat16* src = zpad;
        if ((unsigned)hi < (unsigned)g.H && (unsigned)wi < (unsigned)HW)
          src = x + (((img * g.H + hi) * HW + wi) << LGCH) + pl * 64 +
                (lane >> 3) * 8;
        __builtin_amdgcn_global_load_lds(
            (const __attribute__((address_space(1))) unsigned int*)src,
            (__attribute__((address_space(3))) unsigned int*)(smem + pc * 512),
            16, 0, 0);
      }
    }
    // per-lane fragment address for each column shift s of a tap
    int abase[3];
#pragma unroll
    for (int st = 0; st < 3; ++st) {
      const int q = frow + st;
      abase[st] = (wm / HW) * HP * 128 + (q >> 3) * 1024 + (q & 7) * 16 +
                  (lane >> 4) * 128;
    }
    __syncthreads();

    // tap-major K, one (tap, 64-channel slice) per 64-deep step: a real loop
    // over the tap rows (fully unrolled, the dgrad epilogue modes spill), the
    // three column shifts and the slices unrolled so that their offsets stay
    // immediates
#pragma unroll 1
    for (int rt = 0; rt < 3; ++rt)
#pragma unroll
    for (int st = 0; st < 3; ++st)
#pragma unroll
    for (int sl = 0; sl < NPL; ++sl) {
      const int kt = (rt * 3 + st) * NPL + sl;
      if (kt + 1 < 9 * NPL) stage_w((kt + 1) & 1, kt + 1);
      const __hip_bfloat16* sb = sw + (kt & 1) * (BN * BK);
      const char* ha = (const char*)smem + sl * (HALO_ELEMS * 2) +
                       rt * (HP * 128) + abase[st];
      bf16x8 bf[NI][2];
#pragma unroll
      for (int ni = 0; ni < NI; ++ni)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          const int row = wn + ni * 16 + frow;
          bf[ni][ks] = *(const bf16x8*)((const char*)(sb + row * BK) +
                                        kswz(row, ks * 64 + fkb));
        }
#pragma unroll
      for (int mi = 0; mi < 8; ++mi) {
        const int cpos = ((mi * 16) / HW) * HP + (mi * 16) % HW;
        bf16x8 af[2];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
          af[ks] = *(const bf16x8*)(ha + cpos * 128 + ks * 512);
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) {
          acc[mi][ni] = mfma16(af[0], bf[ni][0], acc[mi][ni]);
          acc[mi][ni] = mfma16(af[1], bf[ni][1], acc[mi][ni]);
        }
      }
      __syncthreads();
    }
  }

  // ---- BN-stats partials (before the bf16 staging): per column, sum and
  // sum-of-squares over the block's BM rows.  C/D map: col = lane&15,
  // row-group = lane>>4 — reduce over the 4 row-groups via shfl.
  if (STATS && stats_ws) {
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
      float sv = 0.f, qv = 0.f;
#pragma unroll
      for (int mi = 0; mi < 8; ++mi)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const float v = acc[mi][ni][reg];
          sv += v;
          qv += v * v;
        }
      sv += __shfl_xor(sv, 16);
      qv += __shfl_xor(qv, 16);
      sv += __shfl_xor(sv, 32);
      qv += __shfl_xor(qv, 32);
      if (lane < 16) {
        const int col = n0 + wn + ni * 16 + frow;
        // big grids always wrap the capped workspace -> atomics
        // (pre-zeroed by the host, same convention as the NT kernel)
        const long long wsrow =
            ((flat_id * NWM + wave / NWN)) % ws_nblocks;
        atomicAdd(&stats_ws[wsrow * N + col], sv);
        atomicAdd(&stats_ws[((long long)ws_nblocks + wsrow) * N + col], qv);
      }
    }
  }

  // ---- epilogue: stage the y tile through LDS for coalesced rows
  __hip_bfloat16* cs = smem;  // [BM][BN] bf16
  constexpr int CPR = BN / 8;        // 16B chunks per row
  constexpr int RPR = THREADS / CPR; // rows per round
  constexpr int NR = BM / RPR;       // store rounds
  const int wrow = tid / CPR, wchunk = tid % CPR;
  // addend / mask chunks ride PF rounds ahead of the store that uses them:
  // the first PF rounds are issued here, so their latency hides behind the
  // LDS staging + barrier; the rest are issued one round at a time inside
  // the store loop (never all NR rounds in registers at once).
  constexpr bool HAS_ADD = (EPI & EPI_ADD) != 0;
  constexpr bool HAS_MASK = (EPI & EPI_MASK) != 0;
  constexpr bool HAS_BNS = (EPI & EPI_BNSTATS) != 0;  // av[] carries t
  constexpr int PF = 2;
  static_assert(NR >= PF, "epilogue prefetch deeper than the store loop");
  short8 av[PF] = {}, mv[PF] = {};
  // y row of a tile row; PAR: dx pixel (n, 2i + pa, 2j + pb) of dy position
  // m0 + row = (n, i, j)
  auto yrow = [&](int row) -> long long {
    if constexpr (PAR) {
      const long long m = m0 + row;
      const int i = (int)(m >> lgW) & (g.H - 1), j = (int)m & (g.W - 1);
      return ((((m >> (lgW + lgH)) << (lgH + 1)) + 2 * i + pa) << (lgW + 1)) +
             2 * j + pb;
    } else {
      return m0 + row;
    }
  };
  auto epi_load = [&](int r, int slot) {
    const long long off =
        (yrow(r * RPR + wrow) * N + n0) * 2 + wchunk * 16;  // bytes
    if constexpr (HAS_ADD || HAS_BNS)
      av[slot] = *(const short8*)((const char*)addend + off);
    if constexpr (HAS_MASK)
      mv[slot] = *(const short8*)((const char*)out_mask + off);
  };
  if constexpr (EPI != EPI_NONE) {
#pragma unroll
    for (int p = 0; p < PF; ++p) epi_load(p, p);
  }
#pragma unroll
  for (int mi = 0; mi < 8; ++mi)
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
      const int col = wn + ni * 16 + frow;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int row = wm + mi * 16 + (lane >> 4) * 4 + reg;
        cs[row * BN + col] = f2bf(acc[mi][ni][reg]);
      }
    }
  // BN-backward sums: a thread's 8 columns are the same in every store round
  // (wchunk), so it keeps 2x8 running sums; mean/rstd are fetched only now,
  // when the MFMA accumulators are dead.
  float mu[8] = {}, rs[8] = {}, sdg[8] = {}, sdb[8] = {};
  if constexpr (HAS_BNS) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      mu[j] = bn_mean[n0 + wchunk * 8 + j];
      rs[j] = bn_rstd[n0 + wchunk * 8 + j];
    }
  }
  __syncthreads();
  if constexpr (!HAS_BNS) {
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int row = r * RPR + wrow;
      short8 c = *(const short8*)((const char*)(cs + row * BN) + wchunk * 16);
      if constexpr (EPI != EPI_NONE) {
        const short8 a = av[r % PF], m = mv[r % PF];
        if (r + PF < NR) epi_load(r + PF, r % PF);
        // same per-element op chain as ew::binary_kernel<bf16, AddOp> then
        // <bf16, ReluBwdOp>: fp32 add, RNE to bf16, then 0 where !(mask > 0)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          short v = c[j];
          if constexpr (HAS_ADD) v = f2bfbits(bfbits2f(v) + bfbits2f(a[j]));
          if constexpr (HAS_MASK)
            v = f2bfbits(bfbits2f(m[j]) > 0.f ? bfbits2f(v) : 0.f);
          c[j] = v;
        }
      }
      *(short8*)((char*)(y + yrow(row) * N + n0) + wchunk * 16) = c;
    }
  } else {
    // Masked store plus the BN-backward sums.  A real loop over pairs of
    // rounds (one per prefetch slot): unrolled like the loop above, the
    // addresses of all NR rounds are formed up front, and with the 32 extra
    // live floats the 256-wide tile spills.
    static_assert(PF == 2 && NR % PF == 0, "store loop steps by slot pairs");
    auto store_round = [&](int r, int slot) {
      const int row = r * RPR + wrow;
      short8 c = *(const short8*)((const char*)(cs + row * BN) + wchunk * 16);
      const short8 t = av[slot], m = mv[slot];
      if (r + PF < NR) epi_load(r + PF, slot);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        // the stored value, exactly as EPI_MASK stores it; the sums use the
        // expression of bn_bwd_stats_kernel
        const float gv = bfbits2f(m[j]) > 0.f ? bfbits2f(c[j]) : 0.f;
        c[j] = f2bfbits(gv);
        sdb[j] += gv;
        sdg[j] += gv * (bfbits2f(t[j]) - mu[j]) * rs[j];
      }
      *(short8*)((char*)(y + yrow(row) * N + n0) + wchunk * 16) = c;
    };
#pragma unroll 1
    for (int r = 0; r < NR; r += PF) {
      store_round(r, 0);
      store_round(r + 1, 1);
    }
  }

  // ---- BN-backward sums: combine the RPR threads that share a column
  // group through LDS (the tile buffer is free once every thread has read
  // its rows), then one atomic per column and sum into the pre-zeroed
  // workspace.  Consecutive lanes add to consecutive columns of one row.
  if constexpr (HAS_BNS) {
    constexpr int P = THREADS / (2 * BN);  // threads per column sum: 4/2/1
    constexpr int RP = RPR / P;            // rows each of them adds (16)
    static_assert(P >= 1 && RP * P == RPR, "column reduction split");
    static_assert((2 * RPR * BN + P * 2 * BN) * sizeof(float) <=
                      sizeof(smem), "reduction buffers exceed the tile LDS");
    float* red = reinterpret_cast<float*>(smem);  // [2][RPR][BN]
    float* red2 = red + 2 * RPR * BN;             // [P][2*BN]
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      red[wrow * BN + wchunk * 8 + j] = sdg[j];
      red[(RPR + wrow) * BN + wchunk * 8 + j] = sdb[j];
    }
    __syncthreads();
    const int ci = tid % (2 * BN), part = tid / (2 * BN);
    const int which = ci / BN, col = ci % BN;  // which: 0 = dg, 1 = db
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < RP; ++i)
      s += red[(which * RPR + part * RP + i) * BN + col];
    if constexpr (P > 1) {
      red2[part * 2 * BN + ci] = s;
      __syncthreads();
      if (part != 0) return;
      s = red2[ci];
#pragma unroll
      for (int p = 1; p < P; ++p) s += red2[p * 2 * BN + ci];
    }
    const long long wsrow = flat_id % ws_nblocks;
    atomicAdd(&stats_ws[((long long)which * ws_nblocks + wsrow) * N + n0 + col],
              s);
  }
}

}  // namespace cg

// BN-backward sums request of a dgrad launch (cg::EPI_BNSTATS): the BN input
// t, its saved mean / rstd, and where to return the workspace.
struct GldsBnStats {
  const torch::Tensor& bn_x;
  const torch::Tensor& mean;
  const torch::Tensor& rstd;
  torch::Tensor ws;  // out: zeroed [2R][C] fp32, R <= kBnStatsRows
};

// Workspace rows of the BN-backward sums: the 1024 rows bn_bwd's own stats
// pass uses at most, so bn_bwd_finalize_kernel runs in the launch shape it
// has today; blocks beyond that wrap (every block adds with atomics).
constexpr int kBnStatsRows = 1024;

// Shape test of the halo-resident A route (cg::conv_fwd_glds_kernel, HW != 0);
// H, W are the input's, which pad 1 / stride 1 make the output's as well.
// Pure host arithmetic — the launcher calls it, and it is exported so that a
// test can tell which route a shape takes.  The LDS budget is the 64-wide
// tile's 80 KB (two blocks per CU): it admits W = 16, 32 and 64.
bool conv_halo64_eligible(int64_t H, int64_t W, int64_t C, int64_t Kout,
                          int64_t R, int64_t S, int64_t stride, int64_t pad) {
  if (R != 3 || S != 3 || stride != 1 || pad != 1 || C != 64) return false;
  if (Kout <= 0 || Kout % 64 || Kout % 128 == 0) return false;  // BN == 64
  if (W < 16 || W % 16 || cg::BM % W) return false;
  const int64_t k = cg::BM / W;  // image rows per 256-row M-tile
  if (k > H || H % k) return false;
  return cg::halo_bytes((int)W) + 2 * 64 * cg::BK * 2 <=
         2 * (cg::BM + 64) * cg::BK * 2;
}

// Shape test of the halo-resident A route of the 128-wide tile (cg::
// conv_fwd_glds_kernel<128, *, *, 16>), same conventions as
// conv_halo64_eligible.  A 256-row M-tile is one 16 x 16 slab of an image, its
// patch two 64-channel planes: C = 128 and W = 16 only (143,360 B of LDS).
bool conv_halo128_eligible(int64_t H, int64_t W, int64_t C, int64_t Kout,
                           int64_t R, int64_t S, int64_t stride, int64_t pad) {
  if (R != 3 || S != 3 || stride != 1 || pad != 1 || C != 128) return false;
  if (Kout <= 0 || Kout % 128 || Kout % 256 == 0) return false;  // BN == 128
  if (W != 16) return false;
  return H >= 16 && H % 16 == 0;
}

// Shape test of the parity-split stride-2 dgrad route (cg::
// conv_fwd_glds_kernel, PAR).  Arguments are the FORWARD conv's: input dims
// H x W (= dx), Cin = dx channels, Kout = dy channels, batch N.  Pure host
// arithmetic, exported like conv_halo64_eligible.  Beyond the 3x3 / stride 2 /
// pad 1 / even H, W form and the glds kernel's own conditions, the dy dims
// H/2 and W/2 must be powers of two: the kernel maps tile rows to pixels with
// shifts (ImageNet-size pyramids, 56 -> 28, keep the stuffed route).
bool conv_dgrad_s2_parity_eligible(int64_t H, int64_t W, int64_t Cin,
                                   int64_t Kout, int64_t R, int64_t S,
                                   int64_t stride, int64_t pad, int64_t N) {
  if (R != 3 || S != 3 || stride != 2 || pad != 1) return false;
  if (N <= 0 || H <= 0 || W <= 0 || (H & 1) || (W & 1)) return false;
  const int64_t HO = H / 2, WO = W / 2;
  if ((HO & (HO - 1)) || (WO & (WO - 1))) return false;
  if (Kout < 64 || (Kout & (Kout - 1))) return false;  // dy channels
  if (Cin <= 0 || Cin % 64) return false;              // dx channels
  const int64_t Mc = N * HO * WO;                      // rows per class
  if (Mc % cg::BM) return false;
  return 4 * (Mc / cg::BM) <= 2147483647LL / 8;
}

// Host entry: returns true when handled.  y must be pre-allocated
// [N,HO,WO,Kout]; stats_ws (optional) pre-zeroed [2*ws_nblocks, Kout].
// addend / out_mask (optional, dgrad only, never with stats_ws): y-shaped
// contiguous tensors applied in the store phase — see cg::EPI_*.
// bns (optional, with out_mask only): also emit the BN-backward sums; the
// zeroed workspace is allocated here, once the shape is known to be taken.
static bool conv2d_glds_launch(const torch::Tensor& x, const torch::Tensor& w,
                               torch::Tensor& y, const torch::Tensor& zp,
                               int64_t stride, int64_t pad, float* stats_ws,
                               int ws_nblocks, int lgSt,
                               const c10::optional<torch::Tensor>& addend,
                               const c10::optional<torch::Tensor>& out_mask,
                               GldsBnStats* bns) {
  static const char* e = getenv("PDT_CONV_GLDS");
  if (e && e[0] == '0') return false;
  if (x.scalar_type() != torch::kBFloat16) return false;
  const int N_ = (int)x.size(0), H = (int)x.size(1), W = (int)x.size(2),
            C = (int)x.size(3);
  const int Kout = (int)w.size(0), R = (int)w.size(1), S = (int)w.size(2);
  if (C < 64 || (C & (C - 1))) return false;
  const int HO = (int)y.size(1), WO = (int)y.size(2);
  const int lgC = log2_exact(C);
  const long long M = (long long)N_ * HO * WO;
  const int K = R * S * C;
  if (Kout % 64) return false;
  const int BN = Kout % 256 == 0 ? 256 : Kout % 128 == 0 ? 128 : 64;
  if (M % cg::BM) return false;
  if (M / cg::BM > 2147483647LL / 8) return false;
  cg::Geom g{H, W, C, lgC, HO, WO, (int)stride, (int)pad, S, R * S, lgSt};
  auto stream = c10::hip::getCurrentHIPStream();
  dim3 grid(Kout / BN, (unsigned)(M / cg::BM));
  const int epi = (addend.has_value() ? cg::EPI_ADD : 0) |
                  (out_mask.has_value() ? cg::EPI_MASK : 0);
  for (const auto* t : {&addend, &out_mask}) {
    if (!t->has_value()) continue;
    TORCH_CHECK(!stats_ws,
                "conv glds: addend/out_mask exclude the stats epilogue");
    TORCH_CHECK((*t)->is_cuda() && (*t)->is_contiguous() &&
                    (*t)->scalar_type() == x.scalar_type() &&
                    (*t)->numel() == y.numel(),
                "conv glds: addend/out_mask must be contiguous, of dy's dtype "
                "and dx-sized");
  }
  const bf16* addp = addend.has_value() ? ptr16<bf16>(*addend) : nullptr;
  const bf16* maskp = out_mask.has_value() ? ptr16<bf16>(*out_mask) : nullptr;
  const float *meanp = nullptr, *rstdp = nullptr;
  if (bns) {
    TORCH_CHECK(epi == cg::EPI_MASK && !stats_ws,
                "conv glds: BN-backward sums need out_mask and no addend");
    TORCH_CHECK(bns->bn_x.is_cuda() && bns->bn_x.is_contiguous() &&
                    bns->bn_x.scalar_type() == x.scalar_type() &&
                    bns->bn_x.numel() == y.numel(),
                "conv glds: bn_x must be contiguous, of dy's dtype and "
                "dx-sized");
    for (const auto* t : {&bns->mean, &bns->rstd})
      TORCH_CHECK(t->is_cuda() && t->is_contiguous() &&
                      t->scalar_type() == torch::kFloat32 &&
                      t->numel() == Kout,
                  "conv glds: bn_mean/bn_rstd must be fp32 [C]");
    ws_nblocks = (int)std::min<long long>(kBnStatsRows,
                                          (long long)grid.x * grid.y);
    bns->ws = torch::zeros({2LL * ws_nblocks, Kout},
                           x.options().dtype(torch::kFloat32));
    stats_ws = bns->ws.data_ptr<float>();
    addp = ptr16<bf16>(bns->bn_x);  // rides in the addend operand slot
    meanp = bns->mean.data_ptr<float>();
    rstdp = bns->rstd.data_ptr<float>();
  }
  // halo-resident A for the 64-channel 3x3 layers; PDT_CONV_HALO64=0 keeps
  // the per-tap gather (read per call, so one process can run both routes)
  const char* eh = getenv("PDT_CONV_HALO64");
  const bool halo = !(eh && eh[0] == '0') && lgSt == 0 && H == HO && W == WO &&
                    conv_halo64_eligible(H, W, C, Kout, R, S, stride, pad);
  // the same on the 128-wide tile (C = 128, W = 16); PDT_CONV_HALO128=0
  const char* eh2 = getenv("PDT_CONV_HALO128");
  const bool halo128 = !(eh2 && eh2[0] == '0') && lgSt == 0 && H == HO &&
                       W == WO &&
                       conv_halo128_eligible(H, W, C, Kout, R, S, stride, pad);
#define CG_HALO(ST, EP)                                       \
  (W == 16   ? &cg::conv_fwd_glds_kernel<64, ST, EP, 16>      \
   : W == 32 ? &cg::conv_fwd_glds_kernel<64, ST, EP, 32>      \
             : &cg::conv_fwd_glds_kernel<64, ST, EP, 64>)
#define CG_KERN(ST, EP)                                       \
  (halo        ? CG_HALO(ST, EP)                              \
   : halo128   ? &cg::conv_fwd_glds_kernel<128, ST, EP, 16>   \
   : BN == 256 ? &cg::conv_fwd_glds_kernel<256, ST, EP>       \
   : BN == 128 ? &cg::conv_fwd_glds_kernel<128, ST, EP>       \
               : &cg::conv_fwd_glds_kernel<64, ST, EP>)
  // parity-split stride-2 dgrad; PDT_DGRAD_S2_PARITY=0 keeps the stuffed
  // gather (read per call).  Here x is dy, y is dx and w the rotated weight
  // [dx channels][R][S][dy channels]; pad is R - 1 - (the forward's pad).
  const char* ep = getenv("PDT_DGRAD_S2_PARITY");
  const bool par = !(ep && ep[0] == '0') && lgSt == 1 && stride == 1 &&
                   (bns || !stats_ws) && HO == 2 * H && WO == 2 * W &&
                   conv_dgrad_s2_parity_eligible(HO, WO, Kout, C, R, S, 2,
                                                 R - 1 - pad, N_);
#define CG_DGRAD(EP)                                                      \
  (!par        ? CG_KERN(false, EP)                                       \
   : BN == 256 ? &cg::conv_fwd_glds_kernel<256, false, EP, 0, true>       \
   : BN == 128 ? &cg::conv_fwd_glds_kernel<128, false, EP, 0, true>       \
               : &cg::conv_fwd_glds_kernel<64, false, EP, 0, true>)
  auto kern = bns                     ? CG_DGRAD(cg::EPI_MASK_BNSTATS)
              : stats_ws              ? CG_KERN(true, cg::EPI_NONE)
              : epi == cg::EPI_NONE   ? CG_DGRAD(cg::EPI_NONE)
              : epi == cg::EPI_ADD    ? CG_DGRAD(cg::EPI_ADD)
              : epi == cg::EPI_MASK   ? CG_DGRAD(cg::EPI_MASK)
                                      : CG_DGRAD(cg::EPI_ADD_MASK);
#undef CG_DGRAD
#undef CG_KERN
#undef CG_HALO
  hipLaunchKernelGGL(kern, grid, dim3(cg::THREADS), 0, stream, ptr16<bf16>(x),
                     ptr16<bf16>(w), ptr16<bf16>(y), ptr16<bf16>(zp), (int)M,
                     Kout, K, g, stats_ws, ws_nblocks, addp, maskp, meanp,
                     rstdp);
  return true;
}

bool conv2d_fwd_glds_ex(const torch::Tensor& x, const torch::Tensor& w,
                        torch::Tensor& y, const torch::Tensor& zp,
                        int64_t stride, int64_t pad, float* stats_ws,
                        int ws_nblocks, int lgSt,
                        const c10::optional<torch::Tensor>& addend,
                        const c10::optional<torch::Tensor>& out_mask) {
  return conv2d_glds_launch(x, w, y, zp, stride, pad, stats_ws, ws_nblocks,
                            lgSt, addend, out_mask, nullptr);
}

// Masked dgrad that also emits the BN-backward sums of the BN it feeds.
// Returns the workspace ([2R][C]: rows [0,R) sum dz*xhat, [R,2R) sum dz), or
// an undefined tensor when the kernel declines the shape (nothing launched).
torch::Tensor conv2d_dgrad_glds_bnstats(
    const torch::Tensor& dy, const torch::Tensor& wr, torch::Tensor& dx,
    const torch::Tensor& zp, int64_t pad, int lgSt,
    const torch::Tensor& out_mask, const torch::Tensor& bn_x,
    const torch::Tensor& bn_mean, const torch::Tensor& bn_rstd) {
  GldsBnStats bns{bn_x, bn_mean, bn_rstd, torch::Tensor()};
  if (!conv2d_glds_launch(dy, wr, dx, zp, 1, pad, nullptr, 0, lgSt,
                          c10::nullopt, out_mask, &bns))
    return torch::Tensor();
  return bns.ws;
}

bool conv2d_fwd_glds(const torch::Tensor& x, const torch::Tensor& w,
                     torch::Tensor& y, const torch::Tensor& zp,
                     int64_t stride, int64_t pad, float* stats_ws,
                     int ws_nblocks) {
  return conv2d_fwd_glds_ex(x, w, y, zp, stride, pad, stats_ws, ws_nblocks,
                            0, c10::nullopt, c10::nullopt);
}
