// Weight gradient of the convolutions of conv_igemm.hip for gfx950 (MI355X): the ONE route decision
// between its three kernels, their split-count rule, the register-staged TT kernel and the reduce.
//   wgrad   : DW[co][tap,ci] = sum_pix DZ[pix][co] * X[src(pix,tap)][ci]           (TT)
// (16-B "chunks" of 8 bf16/f16 or 4 f32 channels along the columns.)  TT tiles are staged as
// [32 pixels][cols] and read with ds_read_b64_tr_b16 (hardware transpose) so both operands get 8
// consecutive pixels per lane.  wgrad is split over pixels into fp32 partial slabs that a second
// kernel reduces deterministically (no atomics); wgrad_ring.hip and wgrad_halo.hip write the same slabs.
#include <algorithm>

#include "wgrad.hpp"
#include "wgrad_halo.hpp"
#include "wgrad_ring.hpp"

namespace yms {

// ---- wgrad: TT GEMM over pixels with ds_read_b64_tr_b16 operands, split-K partial slabs ----
struct TTParams {
  const char* x;
  const char* dz;
  float* slab;
  int x_ld, x_off, dz_ld, dz_off;
  int SH, SW, OW, stride, pad;
  int cpt;       // chunks per tap of x channels
  int Kc;        // valid kf chunks
  int M;         // pixels (rows of dz)
  int cout8;     // cout rounded up to 8 (valid dz channels incl. zero pad)
  int nkt;       // pixel tiles of KP
  uint32_t dz_bytes, x_bytes;   // raw-buffer extents of dz and x (< 2^31)
  int kt_per_split;
  int tiles_n;   // kf tiles
  int tiles_m_n; // row tiles x kf tiles
  int slab_rows, slab_ld;
  FastDiv div_ow, div_ohw;
};

// raw-buffer 16-B load into registers; an offset at or past num_records returns zeros
// (device-only wrapper, see blds16)
__device__ __forceinline__ u32x4 bld16(__amdgpu_buffer_rsrc_t r, uint32_t voff) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(r, voff, 0, 0));
#else
  (void)r; (void)voff;
  return u32x4{0u, 0u, 0u, 0u};
#endif
}

// KP pixels per k-tile, NW waves per block, OCC blocks per CU.  Operands are register-staged
// through raw-buffer loads (out-of-image / out-of-range lanes read zeros: no branches, 32-bit
// offsets) into padded LDS images consumed by the transposing ds_read_b64_tr_b16.
template <typename T, int KS, int BM, int BN, int KP, int NW, int OCC>
__global__ __launch_bounds__(NW * 64, OCC) void conv_wgrad_kernel(TTParams p) {
  constexpr int NTHR = NW * 64;
  // 32- and 96-row tiles (cout <= 32, <= 96) lay all waves along the kf columns
  constexpr int WGN = (BM == 32 || BM == 96) ? NW : (NW == 8 && BN >= 128) ? 4 : 2, WGM = NW / WGN;
  constexpr int WTM = BM / WGM, WTN = BN / WGN;
  constexpr int TM = WTM / 32, TN = WTN / 32;
  static_assert(TM >= 1 && TN >= 1 && WTM % 32 == 0 && WTN % 32 == 0 && KP % 16 == 0, "wgrad tile");
  constexpr int SZ = sizeof(T);
  constexpr bool F32 = SZ == 4;
  constexpr int EPC = 16 / SZ;                 // elements per chunk
  // LDS pitches (conflict-free tr reads: a pitch that is a multiple of the 256-B bank span
  // would put the 4 rows one tr-read group touches on the same banks)
  constexpr int PA = BM * SZ + ((BM * SZ + 64) % 256 == 0 ? 128 : 64), PB = BN * SZ + 64;
  constexpr int CA = BM / EPC, CB = BN / EPC;  // chunks per LDS row
  constexpr int A_SLOTS = (KP * CA + NTHR - 1) / NTHR, B_SLOTS = (KP * CB + NTHR - 1) / NTHR;
  constexpr int TILE = KP * (PA + PB);
  __shared__ __attribute__((aligned(16))) char smem[2 * TILE];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WGN, wn = wave % WGN;
  // 1-D grid, split-major logical order: the tiles sharing a pixel split (its dz rows and x
  // im2col columns) are consecutive logical ids, which xcd_remap keeps on one XCD's L2
  const int tmn = p.tiles_m_n;
  // (measured: grouping pays from 4 tiles per split up; below that plain dispatch order is faster)
  const int lid = tmn >= 4 ? xcd_remap(blockIdx.x, gridDim.x) : (int)blockIdx.x;
  const int wg = lid % tmn;
  const int tile_n = wg % p.tiles_n, tile_m = wg / p.tiles_n;
  const int split = lid / tmn;
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  const int kt0 = split * p.kt_per_split;
  const int kt1 = min(p.nkt, kt0 + p.kt_per_split);

  const __amdgpu_buffer_rsrc_t rs_a =
      __builtin_amdgcn_make_buffer_rsrc((void*)p.dz, (short)0, (int)p.dz_bytes, NT_RSRC3);
  const __amdgpu_buffer_rsrc_t rs_b =
      __builtin_amdgcn_make_buffer_rsrc((void*)p.x, (short)0, (int)p.x_bytes, NT_RSRC3);
  const uint32_t dz_row = (uint32_t)(p.dz_ld * SZ);
  // A-side (dz) slots: fixed pixel row within the k-tile and fixed channel chunk
  int a_row[A_SLOTS];
  uint32_t a_col[A_SLOTS];
#pragma unroll
  for (int i = 0; i < A_SLOTS; ++i) {
    const int c = tid + NTHR * i;
    a_row[i] = c / CA;
    const int ch = m0 + (c - a_row[i] * CA) * EPC;
    a_col[i] = (c < KP * CA && ch < p.cout8) ? (uint32_t)((p.dz_off + ch) * SZ) : NT_OOB;
  }
  // B-side (x im2col) chunk columns are fixed per slot: precompute tap decomposition.
  int b_row[B_SLOTS], b_kh[B_SLOTS], b_kw[B_SLOTS], b_cc[B_SLOTS], b_col[B_SLOTS];
  bool b_kok[B_SLOTS];
#pragma unroll
  for (int j = 0; j < B_SLOTS; ++j) {
    const int c = tid + NTHR * j;
    b_row[j] = c / CB;
    b_col[j] = c - b_row[j] * CB;
    const int kc = n0 / EPC + b_col[j];
    b_kok[j] = (c < KP * CB) && kc < p.Kc;
    const int t = kc / p.cpt;
    b_cc[j] = kc - t * p.cpt;
    b_kh[j] = t / KS;
    b_kw[j] = t - b_kh[j] * KS;
  }
  u32x4 a_reg[A_SLOTS], b_reg[B_SLOTS];

  auto load_tile = [&](int kt) {
    const int q0 = kt * KP;
#pragma unroll
    for (int i = 0; i < A_SLOTS; ++i) {
      const int qpix = q0 + a_row[i];
      const bool ok = a_col[i] != NT_OOB && qpix < p.M;
      a_reg[i] = bld16(rs_a, ok ? (uint32_t)qpix * dz_row + a_col[i] : NT_OOB);
    }
#pragma unroll
    for (int j = 0; j < B_SLOTS; ++j) {
      const int qpix = q0 + b_row[j];
      bool ok = b_kok[j] && qpix < p.M;
      const uint32_t mm = ok ? (uint32_t)qpix : 0u;
      const uint32_t n = fdiv(mm, p.div_ohw);
      const uint32_t rem = mm - n * p.div_ohw.d;
      const uint32_t oy = fdiv(rem, p.div_ow);
      const uint32_t ox = rem - oy * p.div_ow.d;
      const int iy = (int)oy * p.stride - p.pad + b_kh[j];
      const int ix = (int)ox * p.stride - p.pad + b_kw[j];
      ok = ok && iy >= 0 && iy < p.SH && ix >= 0 && ix < p.SW;
      const uint32_t e = (uint32_t)((((int)n * p.SH + iy) * p.SW + ix) * p.x_ld + p.x_off);
      b_reg[j] = bld16(rs_b, ok ? e * SZ + (uint32_t)(b_cc[j] * 16) : NT_OOB);
    }
  };
  auto store_tile = [&](int buf) {
    char* A = smem + buf * TILE;
    char* B = A + KP * PA;
#pragma unroll
    for (int i = 0; i < A_SLOTS; ++i) {
      const int c = tid + NTHR * i;
      if (c < KP * CA) *reinterpret_cast<u32x4*>(A + (c / CA) * PA + (c % CA) * 16) = a_reg[i];
    }
#pragma unroll
    for (int j = 0; j < B_SLOTS; ++j) {
      const int c = tid + NTHR * j;
      if (c < KP * CB) *reinterpret_cast<u32x4*>(B + b_row[j] * PB + b_col[j] * 16) = b_reg[j];
    }
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int a = 0; a < TM; ++a)
#pragma unroll
    for (int b = 0; b < TN; ++b)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[a][b][i] = 0.0f;

  const int lr = lane & 31, lh = lane >> 5;
  // tr-read lane geometry (16-lane groups): group g, block row qq, column quad pp
  const int g = lane >> 4, gi = lane & 15, qq = gi >> 2, pp = gi & 3;
  const int th = g >> 1, tcb = 16 * (g & 1);

  auto compute = [&](int buf) {
    const char* A = smem + buf * TILE;
    const char* B = A + KP * PA;
    if constexpr (!F32) {
#pragma unroll
      for (int s = 0; s < KP / 16; ++s) {
        u32x4 af[TM], bfr[TN];
#pragma unroll
        for (int a = 0; a < TM; ++a) {
          const int col = wm * WTM + a * 32 + tcb + 4 * pp;
          const int row = 16 * s + 8 * th + qq;
          const YMS_LDS s16x4* p0 = (const YMS_LDS s16x4*)(A + row * PA + col * 2);
          const YMS_LDS s16x4* p1 = (const YMS_LDS s16x4*)(A + (row + 4) * PA + col * 2);
          s16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((YMS_LDS s16x4*)p0);
          s16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((YMS_LDS s16x4*)p1);
          uint2 u0 = __builtin_bit_cast(uint2, v0), u1 = __builtin_bit_cast(uint2, v1);
          af[a] = u32x4{u0.x, u0.y, u1.x, u1.y};
        }
#pragma unroll
        for (int b = 0; b < TN; ++b) {
          const int col = wn * WTN + b * 32 + tcb + 4 * pp;
          const int row = 16 * s + 8 * th + qq;
          const YMS_LDS s16x4* p0 = (const YMS_LDS s16x4*)(B + row * PB + col * 2);
          const YMS_LDS s16x4* p1 = (const YMS_LDS s16x4*)(B + (row + 4) * PB + col * 2);
          s16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((YMS_LDS s16x4*)p0);
          s16x4 v1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((YMS_LDS s16x4*)p1);
          uint2 u0 = __builtin_bit_cast(uint2, v0), u1 = __builtin_bit_cast(uint2, v1);
          bfr[b] = u32x4{u0.x, u0.y, u1.x, u1.y};
        }
#pragma unroll
        for (int a = 0; a < TM; ++a)
#pragma unroll
          for (int b = 0; b < TN; ++b) acc[a][b] = Mfma<T>::mma(af[a], bfr[b], acc[a][b]);
      }
    } else {
#pragma unroll
      for (int j = 0; j < KP / 2; ++j) {
        float av[TM], bv[TN];
#pragma unroll
        for (int a = 0; a < TM; ++a)
          av[a] = *reinterpret_cast<const float*>(A + (2 * j + lh) * PA + (wm * WTM + a * 32 + lr) * 4);
#pragma unroll
        for (int b = 0; b < TN; ++b)
          bv[b] = *reinterpret_cast<const float*>(B + (2 * j + lh) * PB + (wn * WTN + b * 32 + lr) * 4);
#pragma unroll
        for (int a = 0; a < TM; ++a)
#pragma unroll
          for (int b = 0; b < TN; ++b)
            acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[a], bv[b], acc[a][b], 0, 0, 0);
      }
    }
  };

  if (kt0 < kt1) {
    load_tile(kt0);
    store_tile(0);
    __syncthreads();
    for (int kt = kt0; kt < kt1; ++kt) {
      const int cur = (kt - kt0) & 1;
      const bool more = kt + 1 < kt1;
      if (more) load_tile(kt + 1);
      compute(cur);
      if (more) store_tile(cur ^ 1);
      __syncthreads();
    }
  }
  float* slab = p.slab + (long)split * p.slab_rows * p.slab_ld;
#pragma unroll
  for (int a = 0; a < TM; ++a)
#pragma unroll
    for (int b = 0; b < TN; ++b)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int row = m0 + wm * WTM + a * 32 + (i & 3) + 8 * (i >> 2) + 4 * lh;
        const int col = n0 + wn * WTN + b * 32 + lr;
        slab[(long)row * p.slab_ld + col] = acc[a][b][i];
      }
}

// dw[co][ci][kh][kw] (+)= sum_s slab[s][co][tap*cin8 + ci].  Block = 32 float4 lanes (128
// consecutive slab columns of one row) x 8 split lanes; every lane keeps two independent
// float4 accumulators, the 8 split lanes are combined through LDS in a fixed order
// (deterministic).  Reads are 16 B/lane, fully coalesced along the slab row.
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* slab, int splits, long slab_elems,
                                                           int slab_ld, int cout, int cin, int cin8, int ks,
                                                           float* dw, int accumulate) {
  __shared__ float4 red[8][33];
  const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
  const int kf = ks * ks * cin8;                // valid slab columns
  const int cpr = (kf + 127) / 128;             // column blocks per row
  const int co = blockIdx.x / cpr;
  const int col = (blockIdx.x - co * cpr) * 128 + lx * 4;
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
  if (col < kf) {
    const float* base = slab + (long)co * slab_ld + col;
    int z = ly;
    for (; z + 8 < splits; z += 16) {
      const float4 u = *reinterpret_cast<const float4*>(base + (long)z * slab_elems);
      const float4 v = *reinterpret_cast<const float4*>(base + (long)(z + 8) * slab_elems);
      a.x += u.x; a.y += u.y; a.z += u.z; a.w += u.w;
      b.x += v.x; b.y += v.y; b.z += v.z; b.w += v.w;
    }
    if (z < splits) {
      const float4 u = *reinterpret_cast<const float4*>(base + (long)z * slab_elems);
      a.x += u.x; a.y += u.y; a.z += u.z; a.w += u.w;
    }
  }
  red[ly][lx] = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
  __syncthreads();
  if (ly == 0 && col < kf) {
    float4 t = red[0][lx];
#pragma unroll
    for (int k = 1; k < 8; ++k) {
      const float4 u = red[k][lx];
      t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w;
    }
    const float tv[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int c = col + e;
      const int tap = c / cin8, ci = c - tap * cin8;
      if (ci < cin) {
        const long o = (((long)co * cin + ci) * ks + tap / ks) * ks + tap % ks;
        dw[o] = accumulate ? dw[o] + tv[e] : tv[e];
      }
    }
  }
}

// ---- host side ----
// Every split writes (and the reduce re-reads) a full fp32 slab of the weight gradient, which on deep
// layers can exceed the layer's own x + dz bytes several times over.  Cap the slab round trip at
// `ratio` x the algorithmic bytes, keeping at least `min_blocks` workgroups.
// (interleaved A/B, YOLOv8-s step: off 19.71/19.71/19.81 ms, ratio 1 19.62/19.64/19.76 ms;
// YOLO-MS-S 40.11/40.12 -> 40.04/40.02 ms -- the wgrads run on the side stream, so the
// step gains only the HBM contention the slabs caused).  Round 4: the step keeps improving down
// to ~0.05, where min_blocks binds (YOLOv8-s 18.23 -> 17.93 ms, YOLO-MS-S 36.22 -> 35.66 ms;
// profiles/r04ad_wgrad_slab_ratio_ab.txt): fewer, longer side-stream blocks and ~no slab bytes.
int wgrad_splits(int by_work, int tiles, int blocks_per_cu, double data_bytes, double slab_rt_bytes) {
  int splits = std::max(1, std::min(by_work, cdiv((long)blocks_per_cu * conv_cu_count(), tiles)));
  const double ratio = env_double("YMS_WG_SLAB_RATIO", 0.05);
  if (ratio > 0.0) {
    const int cap = std::max((int)(ratio * data_bytes / slab_rt_bytes), cdiv(256, tiles));   // min_blocks = 256
    splits = std::max(1, std::min(splits, cap));
  }
  return splits;
}

struct WgradPlan {
  int bm, bn, tiles_m, tiles_n, nkt, want_splits, slab_rows, slab_ld, cin8, cpt, kc, kp;
};
static WgradPlan wgrad_plan(const yms_conv_shape* s) {
  WgradPlan w;
  const int es = elem_size(s->dtype);
  w.cin8 = (int)rup(s->cin, 8);
  w.cpt = w.cin8 * es / 16;
  w.kc = s->k * s->k * w.cpt;
  const int kf = s->k * s->k * w.cin8;
  w.bm = s->cout <= 32 ? 32 : s->cout <= 64 ? 64 : s->cout <= 96 ? 96 : 128;
  w.bn = kf <= 64 ? 64 : 128;
  w.tiles_m = cdiv(s->cout, w.bm);
  w.tiles_n = cdiv(kf, w.bn);
  w.slab_rows = w.tiles_m * w.bm;
  w.slab_ld = w.tiles_n * w.bn;
  w.kp = 32;
  const long M = (long)s->n * s->ho * s->wo;
  w.nkt = cdiv(M, w.kp);
  // about 4 workgroups per CU (2-4 resident by LDS), at least 512 pixels per split
  const double data = (double)M * (double)(rup(s->cout, 8) + w.cin8) * es;
  const double slab_rt = 2.0 * 4.0 * (double)w.slab_rows * (double)w.slab_ld;
  w.want_splits = wgrad_splits(cdiv(w.nkt, 512 / w.kp), w.tiles_m * w.tiles_n, 4, data, slab_rt);
  return w;
}

template <typename T, int KS, int KP, int NW, int OCC>
static void launch_wgrad_v(const TTParams& p, int bm, int bn, dim3 grid, hipStream_t st) {
  // 32-row tiles: 2 / 4 waves of 32 x 32 along kf; 64-row tiles keep 4 waves (2 x 2)
  if (bm == 32 && bn == 64)
    hipLaunchKernelGGL((conv_wgrad_kernel<T, KS, 32, 64, KP, 2, OCC>), grid, dim3(128), 0, st, p);
  else if (bm == 32)
    hipLaunchKernelGGL((conv_wgrad_kernel<T, KS, 32, 128, KP, 4, OCC>), grid, dim3(256), 0, st, p);
  else if (bm == 96 && bn == 64)   // (its registers allow 3 blocks per SIMD's worth, not 4)
    hipLaunchKernelGGL((conv_wgrad_kernel<T, KS, 96, 64, KP, 2, (OCC > 3 ? 3 : OCC)>), grid, dim3(128), 0, st, p);
  else if (bm == 96)
    hipLaunchKernelGGL((conv_wgrad_kernel<T, KS, 96, 128, KP, 4, OCC>), grid, dim3(256), 0, st, p);
  else if (bm == 64 && bn == 64)
    hipLaunchKernelGGL((conv_wgrad_kernel<T, KS, 64, 64, KP, 4, OCC>), grid, dim3(256), 0, st, p);
  else if (bm == 64)
    hipLaunchKernelGGL((conv_wgrad_kernel<T, KS, 64, 128, KP, 4, OCC>), grid, dim3(256), 0, st, p);
  else if (bn == 64)
    hipLaunchKernelGGL((conv_wgrad_kernel<T, KS, 128, 64, KP, NW, OCC>), grid, dim3(NW * 64), 0, st, p);
  else
    hipLaunchKernelGGL((conv_wgrad_kernel<T, KS, 128, 128, KP, NW, OCC>), grid, dim3(NW * 64), 0, st, p);
}

// (round 3, measured and dropped: 64-pixel k-tiles, 8-wave blocks, 3-4 blocks per CU)
template <typename T, int KS>
static void launch_wgrad(const TTParams& p, int bm, int bn, dim3 grid, hipStream_t st) {
  launch_wgrad_v<T, KS, 32, 4, 2>(p, bm, bn, grid, st);
}

static yms_status wgrad_tt_launch(const yms_conv_shape* s, const WgradPlan& w, const WgradArgs& a, hipStream_t st) {
  TTParams p{};
  if (!wgrad_operands(p, s, a)) return YMS_ERR_UNSUPPORTED;
  p.SH = s->h; p.SW = s->w; p.OW = s->wo; p.stride = s->stride; p.pad = s->pad;
  p.cpt = w.cpt; p.Kc = w.kc;
  p.M = s->n * s->ho * s->wo;
  p.cout8 = (int)rup(s->cout, 8);
  p.nkt = w.nkt; p.kt_per_split = a.per; p.tiles_n = w.tiles_n; p.tiles_m_n = w.tiles_m * w.tiles_n;
  p.slab_rows = w.slab_rows; p.slab_ld = w.slab_ld;
  p.div_ow = make_fastdiv(s->wo);
  p.div_ohw = make_fastdiv(s->ho * s->wo);
  dim3 grid((unsigned)(w.tiles_m * w.tiles_n * a.splits));
  if (s->dtype == YMS_BF16) {
    if (s->k == 1) launch_wgrad<bf16, 1>(p, w.bm, w.bn, grid, st); else launch_wgrad<bf16, 3>(p, w.bm, w.bn, grid, st);
  } else if (s->dtype == YMS_F16) {
    if (s->k == 1) launch_wgrad<f16, 1>(p, w.bm, w.bn, grid, st); else launch_wgrad<f16, 3>(p, w.bm, w.bn, grid, st);
  } else {
    if (s->k == 1) launch_wgrad<float, 1>(p, w.bm, w.bn, grid, st); else launch_wgrad<float, 3>(p, w.bm, w.bn, grid, st);
  }
  return launch_status();
}

// The ONE route decision of a weight gradient: yms_conv_wgrad_ws_bytes and yms_conv_wgrad both read it.
struct WgradRoute {
  // HALO: 3x3, each input patch staged once for all nine taps (wgrad_halo.hip); RING: 1x1 / 3x3 with > 32 output
  // channels, both operands on an LDS-DMA ring (wgrad_ring.hip); TT: conv_wgrad_kernel, fp32 and whatever they decline
  enum Kind { TT, RING, HALO } kind;
  int units, per, splits;        // work units (k-tiles / patches), units per split, splits
  int slabs_per_split;           // 1; the halo kernel's 32-output-channel variant: wk = 2
  int slab_rows, slab_ld, cin8;  // one fp32 slab, as wgrad_reduce_kernel reads it
  WgradPlan tt; WRPlan ring; WHPlan halo;   // launch geometry: only the one `kind` names is filled
  size_t split_bytes() const { return (size_t)slabs_per_split * slab_rows * slab_ld * sizeof(float); }
};
static WgradRoute wgrad_route(const yms_conv_shape* s) {
  WgradRoute r{};
  r.slabs_per_split = 1; r.cin8 = (int)rup(s->cin, 8);
  int want;                      // the planner's split count, before it is evened out over the units
  if (wgrad_halo_plan(s, &r.halo)) {
    r.kind = WgradRoute::HALO; r.units = r.halo.npatch; want = r.halo.want_splits; r.slabs_per_split = r.halo.wk;
    r.slab_rows = r.halo.slab_rows; r.slab_ld = r.halo.slab_ld;
  } else if (wgrad_ring_plan(s, &r.ring)) {
    r.kind = WgradRoute::RING; r.units = r.ring.nkt; want = r.ring.want_splits;
    r.slab_rows = r.ring.slab_rows; r.slab_ld = r.ring.slab_ld;
  } else {
    r.tt = wgrad_plan(s);
    r.kind = WgradRoute::TT; r.units = r.tt.nkt; want = r.tt.want_splits;
    r.slab_rows = r.tt.slab_rows; r.slab_ld = r.tt.slab_ld;
  }
  r.per = cdiv(r.units, want);
  r.splits = cdiv(r.units, r.per);
  return r;
}

// fewer split-K partial slabs when the caller's workspace holds fewer than the plan asks for (a
// workspace sized under other YMS_WG_* settings than the call's): units of work (patches / k-tiles)
// per split grow until `splits` slabs of slab_bytes fit; false when not even one fits
static bool fit_splits(size_t ws_bytes, size_t slab_bytes, int units, int& per, int& splits) {
  const size_t cap = ws_bytes / slab_bytes;
  if (cap < 1) return false;
  if ((size_t)splits > cap) {
    per = cdiv(units, (int)cap);
    splits = cdiv(units, per);
  }
  return true;
}

}  // namespace yms

using namespace yms;

extern "C" {

size_t yms_conv_wgrad_ws_bytes(const yms_conv_shape* s) {
  if (!shape_ok(s)) return 0;
  const WgradRoute r = wgrad_route(s);
  return (size_t)r.splits * r.split_bytes();
}

yms_status yms_conv_wgrad(const yms_conv_shape* s, const void* x, int x_ld, int x_off,
                          const void* dz, int dz_ld, int dz_off, float* ws, size_t ws_bytes,
                          float* dw, int accumulate, void* stream) {
  if (!shape_ok(s) || !x || !dz || !ws || !dw) return YMS_ERR_INVALID;
  if (!view_ok(x_ld, x_off, s->cin) || !view_ok(dz_ld, dz_off, s->cout)) return YMS_ERR_INVALID;
  WgradRoute r = wgrad_route(s);
  if (!fit_splits(ws_bytes, r.split_bytes(), r.units, r.per, r.splits)) return YMS_ERR_INVALID;
  const WgradArgs a{x, dz, x_ld, x_off, dz_ld, dz_off, ws, r.per, r.splits};
  hipStream_t st = (hipStream_t)stream;
  yms_status e = YMS_OK;
  switch (r.kind) {
    case WgradRoute::HALO: e = wgrad_halo_launch(s, r.halo, a, st); break;
    case WgradRoute::RING: e = wgrad_ring_launch(s, r.ring, a, st); break;
    case WgradRoute::TT: e = wgrad_tt_launch(s, r.tt, a, st); break;
  }
  if (e != YMS_OK) return e;
  const int kf = s->k * s->k * r.cin8;
  dim3 g2((unsigned)(s->cout * cdiv(kf, 128)));
  hipLaunchKernelGGL(wgrad_reduce_kernel, g2, dim3(256), 0, st, ws, r.splits * r.slabs_per_split,
                     (long)r.slab_rows * r.slab_ld, r.slab_ld, s->cout, s->cin, r.cin8, s->k, dw, accumulate);
  return launch_status();
}

}  // extern "C"
