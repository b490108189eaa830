// BatchNorm / SiLU / residual, SPPF pooling, nearest-x2 upsample and layout kernels for the
// YOLOv8 hot path on gfx950.  All are HBM-bound streaming kernels: 16-B vectorised NHWC
// accesses (8 channels per item), grid-stride loops, fp32 math, deterministic reductions
// (per-block partial rows reduced in a fixed order, fp64 final sums).
//
// Reference semantics (paths relative to rafaelghiorzi/YOLO-MS):
//   nn.BatchNorm2d(eps=1e-3, momentum=0.03) + nn.SiLU   yolov8/model/components.py:72-77
//   Bottleneck residual (always on)                     yolov8/model/components.py:87-93
//   SPPF: three chained MaxPool2d(5, 1, 2) + cat        yolov8/model/components.py:136-146
//   Upsample nearest x2                                 yolov8/model/components.py:159-160
#include <cstdlib>
#include <algorithm>
#include <vector>

#include "yms_common.hpp"

namespace yms {

static inline unsigned grid_for(long items, int block = 256, long cap = 16384) {
  long g = (items + block - 1) / block;
  if (g < 1) g = 1;
  return (unsigned)std::min(g, cap);
}

// ------------------------------------------------------------------------------------------
// BN fold (eval) and finalize (train)
// ------------------------------------------------------------------------------------------
__global__ void bn_fold_kernel(int c, const float* g, const float* b, const float* rm,
                               const float* rv, float eps, float* scale, float* shift) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= c) return;
  if (!g) {  // bias-only (plain nn.Conv2d)
    scale[i] = 1.0f;
    shift[i] = b ? b[i] : 0.0f;
    return;
  }
  const float sc = g[i] / sqrtf(rv[i] + eps);
  scale[i] = sc;
  shift[i] = b[i] - rm[i] * sc;
}

// The fold of a BatchNorm2d in eval mode inside a TRAINING step: scale / shift exactly as bn_fold_kernel
// (so the layer's forward is bit-identical to the eval plan's), plus the (running_mean, invstd) table
// the BN backward passes read in place of the batch statistics.  One job per layer, blockIdx.y = job;
// the outputs are byte offsets from `base` (the step's arena), so one device table serves every step.
struct FoldJob {
  const float *g, *b, *rm, *rv;
  float eps;
  int c, mi_ld;
  long scale, shift, mi;
};
__global__ void bn_fold_mi_kernel(const FoldJob* jobs, const FoldJob solo, char* base) {   // jobs NULL: solo, base 0
  const FoldJob j = jobs ? jobs[blockIdx.y] : solo;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= j.c) return;
  const float sc = j.g[i] / sqrtf(j.rv[i] + j.eps);
  reinterpret_cast<float*>(base + j.scale)[i] = sc;
  reinterpret_cast<float*>(base + j.shift)[i] = j.b[i] - j.rm[i] * sc;
  float* mi = reinterpret_cast<float*>(base + j.mi);
  mi[i] = j.rm[i];
  mi[j.mi_ld + i] = 1.0f / sqrtf(j.rv[i] + j.eps);
}

// Statistics rows (conv_common.hpp contract): row r = (sum z, sum (z - mean_r)^2) over n_r
// pixels, n_r = counts[r] (the producers write the count table right after the rows; rows with
// n_r = 0 are skipped).  Rows are merged in ONE pass in fp64 with the shifted-data form of
// Chan's update: with K = the first row's mean (a sample of the data, so |mean - K| is of the
// order of the spread),  M2 = sum_r [M2_r + n_r (m_r - K)^2] - (sum_r n_r (m_r - K))^2 / N,
// free of the sum z^2 - n mean^2 cancellation.  Row means m_r are formed in fp32 (the
// producers' own precision).
struct Moments {           // n, sum n_r (m_r - K), sum [M2_r + n_r (m_r - K)^2] about the shift K
  double n = 0.0, d1 = 0.0, d2 = 0.0, K = 0.0;
  __device__ void add_row(float s1, float m2, float nr) {
    if (!(nr > 0.f)) return;
    const float mr = s1 / nr;
    if (n == 0.0) K = (double)mr;
    const double d = (double)mr - K;
    n += nr;
    d1 += nr * d;
    d2 += (double)m2 + nr * d * d;
  }
  __device__ void merge(const Moments& o) {      // re-centre o on this K, then add
    if (o.n == 0.0) return;
    if (n == 0.0) { *this = o; return; }
    const double e = o.K - K;
    n += o.n;
    d1 += o.d1 + o.n * e;
    d2 += o.d2 + 2.0 * e * o.d1 + o.n * e * e;
  }
  __device__ double sum() const { return d1 + n * K; }
  __device__ double m2() const { return n > 0.0 ? d2 - d1 * d1 / n : 0.0; }
  __device__ void store(double (*red)[4], int i) const { red[i][0] = n; red[i][1] = d1; red[i][2] = d2; red[i][3] = K; }
  __device__ static Moments load(const double (*red)[4], int i) {
    Moments m;
    m.n = red[i][0]; m.d1 = red[i][1]; m.d2 = red[i][2]; m.K = red[i][3];
    return m;
  }
};

// Grouped launches of the passes below: up to BN_GROUP_MAX independent jobs in one launch.  The
// blocks of member j are [first[j], first[j + 1]) of blockIdx.x, so member j's block
// blockIdx.x - first[j] of first[j + 1] - first[j] does exactly what that block of its solo launch
// does (same pixel range, same partial row): only the number of launches changes.
constexpr int BN_GROUP_MAX = 8;
template <typename Job>
struct BnGroup {
  Job job[BN_GROUP_MAX];
  unsigned first[BN_GROUP_MAX + 1];
  int n;
};
template <typename Job>
__device__ __forceinline__ int group_member(const BnGroup<Job>& g, unsigned& bid, unsigned& nblk) {
  int j = 0;
  while (j + 1 < g.n && blockIdx.x >= g.first[j + 1]) ++j;
  bid = blockIdx.x - g.first[j];
  nblk = g.first[j + 1] - g.first[j];
  return j;
}

// Pre-reduction for long statistics tables: block (cb, s) merges rows [s*R, (s+1)*R) of
// channels [64cb, 64cb+64) and stores the merged (sum, M2) over row s*R -- the first row of its
// own range, so no block reads a row another block writes (the count table is left as it is:
// the finalize sums the counts of each merged range).  256 threads = 64 channels x 4 lanes, two
// rows in flight per lane.
__global__ __launch_bounds__(256) void bn_stats_partial_kernel(int c, float* stats, int rows, int ld, int R) {
  __shared__ double red[4 * 64][4];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int ch = blockIdx.x * 64 + tx;
  const int r0 = blockIdx.y * R, r1 = min(rows, r0 + R);
  const float* cnt = stats + (long)rows * 2 * ld;
  const float* s1p = stats + ch;
  const float* m2p = stats + ld + ch;
  const long rs = 2l * ld;
  Moments a, b;
  if (ch < c) {
    int r = r0 + ty;
    for (; r + 4 < r1; r += 8) {
      a.add_row(s1p[r * rs], m2p[r * rs], cnt[r]);
      b.add_row(s1p[(r + 4) * rs], m2p[(r + 4) * rs], cnt[r + 4]);
    }
    if (r < r1) a.add_row(s1p[r * rs], m2p[r * rs], cnt[r]);
    a.merge(b);
  }
  a.store(red, ty * 64 + tx);
  __syncthreads();
  if (ty == 0 && ch < c) {
    Moments t = Moments::load(red, tx);
    for (int k = 1; k < 4; ++k) t.merge(Moments::load(red, k * 64 + tx));
    stats[(long)r0 * rs + ch] = (float)t.sum();
    stats[(long)r0 * rs + ld + ch] = (float)t.m2();
  }
}

// rows are read at stride rs (rs > 1 after bn_stats_partial_kernel; merged row k covers original
// rows [k*rs, min(rows_total, (k+1)*rs)), its count the sum of theirs); FIN_CW channels x FIN_RL
// row lanes per block (1024 threads: short tables are latency-bound, so many lanes with few
// rows each), one shifted pass per lane, fixed-order tree combine
constexpr int FIN_CW = 8, FIN_RL = 1024 / FIN_CW;
__global__ __launch_bounds__(1024) void bn_finalize_kernel(int c, const float* stats, int rows, int ld, int rs,
                                                           int rows_total, long count, const float* g,
                                                           const float* b, float* rm, float* rv, float momentum,
                                                           float eps, float* mi, int mi_ld, float* scale,
                                                           float* shift) {
  __shared__ double red[FIN_RL * (FIN_CW + 1)][4];
  const int tx = threadIdx.x % FIN_CW, ty = threadIdx.x / FIN_CW;
  const int ch = blockIdx.x * FIN_CW + tx;
  const float* cnt = stats + (long)rows_total * 2 * ld;
  Moments a;
  if (ch < c) {
    if (rs == 1) {
      // four rows per iteration, every load issued before the first use
      int r = ty;
      for (; r + 3 * FIN_RL < rows; r += 4 * FIN_RL) {
        float s1[4], m2[4], n[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          s1[u] = stats[(long)(r + FIN_RL * u) * 2 * ld + ch];
          m2[u] = stats[(long)(r + FIN_RL * u) * 2 * ld + ld + ch];
          n[u] = cnt[r + FIN_RL * u];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) a.add_row(s1[u], m2[u], n[u]);
      }
      for (; r < rows; r += FIN_RL) a.add_row(stats[(long)r * 2 * ld + ch], stats[(long)r * 2 * ld + ld + ch], cnt[r]);
    } else {
      for (int r = ty; r < rows; r += FIN_RL) {
        float n = 0.f;   // integer-valued: exact in fp32 below 2^24 pixels per merged row
        for (int q = r * rs, e = min(rows_total, (r + 1) * rs); q < e; ++q) n += cnt[q];
        a.add_row(stats[(long)r * rs * 2 * ld + ch], stats[(long)r * rs * 2 * ld + ld + ch], n);
      }
    }
  }
  // fixed-order tree over the row lanes: lane ty absorbs lane ty + h
  for (int h = FIN_RL / 2; h >= 1; h >>= 1) {
    if (ty >= h && ty < 2 * h) a.store(red, ty * (FIN_CW + 1) + tx);
    __syncthreads();
    if (ty < h) a.merge(Moments::load(red, (ty + h) * (FIN_CW + 1) + tx));
    __syncthreads();
  }
  if (ty == 0 && ch < c) {
    const double mean = a.n > 0.0 ? a.sum() / a.n : 0.0;
    const double var = fmax(a.m2(), 0.0) / (double)count;
    const float invstd = (float)(1.0 / sqrt(var + (double)eps));
    const double uvar = count > 1 ? var * (double)count / (double)(count - 1) : var;
    if (rm) rm[ch] = (float)((1.0 - momentum) * (double)rm[ch] + momentum * mean);
    if (rv) rv[ch] = (float)((1.0 - momentum) * (double)rv[ch] + momentum * uvar);
    mi[ch] = (float)mean;
    mi[mi_ld + ch] = invstd;
    const float sc = g[ch] * invstd;
    scale[ch] = sc;
    shift[ch] = b[ch] - (float)mean * sc;
  }
}

// Forward finalize for tables of <= 1024 rows (rs == 1), latency-shaped: 8 channels x 32 row
// lanes (256 threads), each lane issues the loads of up to 8 rows at a time (24 in flight) and
// folds them with the same shifted fp64 update; a 5-level fixed-order tree over the lanes (the
// 1024-thread kernel above runs a 7-level tree with two barriers per level).  In the forward no
// side-stream work competes for CU slots, so the finalize's latency is the step's.  Measured
// step-neutral to slightly faster (YOLOv8-s 18.71 / 18.71 -> 18.67 / 18.74 ms, YOLO-MS-S 37.29 /
// 37.37 -> 37.24 / 37.26 ms, profiles/r03u_bn_finalize_small_ab.txt).
constexpr int FIN3_RL = 32;
__device__ __forceinline__ void bn_finalize_small_body(int c, const float* stats, int rows, int ld, long count,
                                                       const float* g, const float* b, float* rm, float* rv,
                                                       float momentum, float eps, float* mi, int mi_ld,
                                                       float* scale, float* shift, const unsigned bid) {
  __shared__ double red[FIN3_RL * 9][4];
  const int tx = threadIdx.x & 7, ty = threadIdx.x >> 3;
  const int ch = bid * 8 + tx;
  const float* cnt = stats + (long)rows * 2 * ld;
  Moments a;
  if (ch < c) {
    for (int r0 = ty; r0 < rows; r0 += FIN3_RL * 8) {
      float s1[8], m2[8], n[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int r = r0 + FIN3_RL * u;
        const bool ok = r < rows;
        s1[u] = ok ? stats[(long)r * 2 * ld + ch] : 0.f;
        m2[u] = ok ? stats[(long)r * 2 * ld + ld + ch] : 0.f;
        n[u] = ok ? cnt[r] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) a.add_row(s1[u], m2[u], n[u]);
    }
  }
  for (int h = FIN3_RL / 2; h >= 1; h >>= 1) {
    if (ty >= h && ty < 2 * h) a.store(red, ty * 9 + tx);
    __syncthreads();
    if (ty < h) a.merge(Moments::load(red, (ty + h) * 9 + tx));
    __syncthreads();
  }
  if (ty == 0 && ch < c) {
    const double mean = a.n > 0.0 ? a.sum() / a.n : 0.0;
    const double var = fmax(a.m2(), 0.0) / (double)count;
    const float invstd = (float)(1.0 / sqrt(var + (double)eps));
    const double uvar = count > 1 ? var * (double)count / (double)(count - 1) : var;
    if (rm) rm[ch] = (float)((1.0 - momentum) * (double)rm[ch] + momentum * mean);
    if (rv) rv[ch] = (float)((1.0 - momentum) * (double)rv[ch] + momentum * uvar);
    mi[ch] = (float)mean;
    mi[mi_ld + ch] = invstd;
    const float sc = g[ch] * invstd;
    scale[ch] = sc;
    shift[ch] = b[ch] - (float)mean * sc;
  }
}
__global__ __launch_bounds__(256) void bn_finalize_small_kernel(int c, const float* stats, int rows, int ld,
                                                                long count, const float* g, const float* b, float* rm,
                                                                float* rv, float momentum, float eps, float* mi,
                                                                int mi_ld, float* scale, float* shift) {
  bn_finalize_small_body(c, stats, rows, ld, count, g, b, rm, rv, momentum, eps, mi, mi_ld, scale, shift, blockIdx.x);
}
struct FinJob {
  int c, rows, ld, mi_ld;
  const float* stats;
  long count;
  const float *g, *b;
  float *rm, *rv;
  float momentum, eps;
  float *mi, *scale, *shift;
};
__global__ __launch_bounds__(256) void bn_finalize_small_group_kernel(BnGroup<FinJob> grp) {
  unsigned bid, nblk;
  const FinJob& j = grp.job[group_member(grp, bid, nblk)];
  bn_finalize_small_body(j.c, j.stats, j.rows, j.ld, j.count, j.g, j.b, j.rm, j.rv, j.momentum, j.eps, j.mi, j.mi_ld,
                         j.scale, j.shift, bid);
}

// ------------------------------------------------------------------------------------------
// Channel-stationary mapping for the per-channel elementwise / reduction kernels:
// G = ceil(C/8) 16-B channel groups, thread (py, g) = (tid / G, tid % G) keeps the same
// 8 channels (and their BN parameters, in registers) for every pixel it visits; the
// PY = 256 / G pixel lanes of a block walk a contiguous pixel range.  One wave-row of a
// pixel is a fully coalesced 16*G-byte segment.  Requires G <= 256 (C <= 2048).
// ------------------------------------------------------------------------------------------
struct ChanMap {
  int G, PY, g, py;
  bool active;
  __device__ ChanMap(int c) {
    G = (c + 7) >> 3;
    PY = 256 / G;
    g = threadIdx.x % G;
    py = threadIdx.x / G;
    active = py < PY;
  }
};

__device__ __forceinline__ void load_params8(const float* p, int c0, int c, float (&v)[8], float dflt) {
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = (p && c0 + i < c) ? p[c0 + i] : dflt;
}

// U pixels per thread per iteration: all U loads issue before any use (memory-level
// parallelism; these kernels are HBM-bound).
constexpr int BN_U = 4;
// the backward reduce / apply passes (8 measured slower: the YOLOv8-s step went 17.80 -> 17.90 ms
// (reduce) and -> 19.43 ms (apply), profiles/r05u_bn_unroll_ab.txt)
constexpr int BN_UR = 4, BN_UA = 4;

// Pixel-range order of the elementwise passes over a tensor: blocks are dispatched in index order,
// so block b taking range nblocks - 1 - b walks the tensor from its end.  A pass that follows one
// which walked the same tensor forward then reads the most recently touched bytes first -- the
// ones still held by the 256 MB memory-side cache -- instead of the ones it evicted first.
// Interleaved A/B (YOLOv8-s B=64 step, 3 reps, profiles/r05r_bn_order_ab.txt): the forward affine
// pass reversed (after the conv that wrote z) 18.22 -> 18.17 ms; also reversing the backward
// reduce or apply gave no more.
constexpr bool BN_REV_AFFINE = true, BN_REV_RED = false, BN_REV_APPLY = false;
// Non-temporal loads where a pass reads a tensor for the last time while the weight gradients run
// beside it (the backward apply's gy and z, the forward affine's z; the reduce's reads stay cached:
// the apply re-reads the same bytes next).  Interleaved A/B (profiles/r06s_bn_nt_ab.txt): YOLOv8-s
// 17.72 -> 17.64 ms/step, YOLO-MS-S 35.56 -> 35.38 ms (each alone gives part of it).
// (bid of nblk: the launch's own block index and grid size, or a grouped launch's member-relative ones)
template <bool REV> __device__ __forceinline__ long block_range(unsigned bid, unsigned nblk) {
  return REV ? (long)(nblk - 1 - bid) : (long)bid;
}

// PIPE (the default): software-pipelined (c % 8 == 0) like the backward passes: the next U pixels' loads
// (clamped to the block's last pixel, masked) are in flight while this U is computed and stored.
template <typename T, bool PIPE>
__device__ __forceinline__ void affine_act_body(long npix, int c, const T* z, int z_ld, int z_off,
                                                const float* scale, const float* shift, int act, const T* res,
                                                int res_ld, int res_off, T* y, int y_ld, int y_off, long ppb,
                                                const unsigned bid, const unsigned nblk) {
  ChanMap m(c);
  if (!m.active) return;
  const int c0 = m.g * 8, nv = min(8, c - c0);
  float sc[8], sh[8];
  load_params8(scale, c0, c, sc, 1.0f);
  load_params8(shift, c0, c, sh, 0.0f);
  const long p0 = block_range<BN_REV_AFFINE>(bid, nblk) * ppb, p1 = min(npix, p0 + ppb);
  auto emit = [&](long pix, const Raw8<T>& zz, const Raw8<T>& rres, int valid) {
    float v[8], r[8];
    unpack8(zz, v);
    if (res) unpack8(rres, r);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      float a = v[i] * sc[i] + sh[i];
      if (act == YMS_ACT_SILU) a = silu_f(a);
      if (res) a += r[i];
      v[i] = a;
    }
    store8(y + pix * y_ld + y_off + c0, valid, v);
  };
  const long step = (long)m.PY * BN_U;
  if (PIPE && c % 8 == 0) {
    auto issue = [&](long b, Raw8<T> (&zz)[BN_U], Raw8<T> (&rres)[BN_U]) {
#pragma unroll
      for (int u = 0; u < BN_U; ++u) {
        const long pix = min(b + (long)u * m.PY, p1 - 1);
        load_raw8_nt(z + pix * z_ld + z_off + c0, zz[u]);       // z's last read until the backward
        if (res) load_raw8(res + pix * res_ld + res_off + c0, 8, rres[u]);
      }
    };
    auto consume = [&](long b, const Raw8<T> (&zz)[BN_U], const Raw8<T> (&rres)[BN_U]) {
#pragma unroll
      for (int u = 0; u < BN_U; ++u) {
        const long pix = b + (long)u * m.PY;
        if (pix < p1) emit(pix, zz[u], rres[u], 8);
      }
    };
    long base = p0 + m.py;
    if (base < p1) {
      Raw8<T> za[BN_U], ra[BN_U], zb[BN_U], rb[BN_U];
      issue(base, za, ra);
      while (true) {
        issue(base + step, zb, rb);
        consume(base, za, ra);
        base += step;
        if (base >= p1) break;
        issue(base + step, za, ra);
        consume(base, zb, rb);
        base += step;
        if (base >= p1) break;
      }
    }
  } else {
    for (long base = p0 + m.py; base < p1; base += step) {
      Raw8<T> zr[BN_U], rr[BN_U];
#pragma unroll
      for (int u = 0; u < BN_U; ++u) {
        const long pix = base + (long)u * m.PY;
        if (pix < p1) {
          load_raw8(z + pix * z_ld + z_off + c0, nv, zr[u]);
          if (res) load_raw8(res + pix * res_ld + res_off + c0, nv, rr[u]);
        }
      }
#pragma unroll
      for (int u = 0; u < BN_U; ++u) {
        const long pix = base + (long)u * m.PY;
        if (pix < p1) emit(pix, zr[u], rr[u], nv);
      }
    }
  }
}
template <typename T, bool PIPE = false>
__global__ __launch_bounds__(256) void affine_act_kernel(long npix, int c, const T* z, int z_ld, int z_off,
                                                         const float* scale, const float* shift, int act,
                                                         const T* res, int res_ld, int res_off, T* y,
                                                         int y_ld, int y_off, long ppb) {
  affine_act_body<T, PIPE>(npix, c, z, z_ld, z_off, scale, shift, act, res, res_ld, res_off, y, y_ld, y_off, ppb,
                           blockIdx.x, gridDim.x);
}
// One elementwise / reduce job of a grouped launch (affine: out = y, res read; reduce: ws; apply:
// out = dz, res = gres; the bias reduce: fin)
struct PassJob {
  long npix, ppb;
  int c, act;
  const void* z; int z_ld, z_off;
  const void* gy; int gy_ld, gy_off;
  const float *scale, *shift, *mi, *coef;
  void* out; int out_ld, out_off;
  void* res; int res_ld, res_off, res_acc;
  float* ws;
};
template <typename T, bool PIPE>
__global__ __launch_bounds__(256) void affine_act_group_kernel(BnGroup<PassJob> grp) {
  unsigned bid, nblk;
  const PassJob& j = grp.job[group_member(grp, bid, nblk)];
  affine_act_body<T, PIPE>(j.npix, j.c, (const T*)j.z, j.z_ld, j.z_off, j.scale, j.shift, j.act, (const T*)j.res,
                           j.res_ld, j.res_off, (T*)j.out, j.out_ld, j.out_off, j.ppb, bid, nblk);
}

// ------------------------------------------------------------------------------------------
// BN + SiLU backward.  Each block owns a contiguous pixel range and writes one partial row
// [2][c] (sum da, sum da*xhat) -- deterministic, no atomics.
// ------------------------------------------------------------------------------------------
struct BwdFin {          // fused finalize (FIN): the last reduce block to finish sums every partial row
  unsigned* cnt;        // arrival counter, zero on entry (the plan zeroes one per layer per backward)
  float *dgamma, *dbeta, *coef;
  long count;
};

// The tail the partial-row kernels share.  block_rows_store: a block's per-thread sums -> its partial row
// [2][c] of ws.  last_block_finish: the in-launch finalize over the nblk rows.
__device__ __forceinline__ void block_rows_store(const ChanMap& m, int c, int c0, const float (&a1)[8],
                                                 const float (&a2)[8], float (&red)[2][2048 + 64], float* ws,
                                                 const long row) {
  // reduce over the PY pixel lanes in a fixed order: red[k][py*8G + g*8 + i]
  const int W = m.G * 8;
  for (int lane0 = 0; lane0 < m.PY; lane0 += 2048 / W) {
    const int lanes = min(m.PY - lane0, 2048 / W);
    if (m.active && m.py >= lane0 && m.py < lane0 + lanes) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        red[0][(m.py - lane0) * W + c0 + i] = a1[i];
        red[1][(m.py - lane0) * W + c0 + i] = a2[i];
      }
    }
    __syncthreads();
    for (int ch = threadIdx.x; ch < c; ch += 256) {
      float t1 = 0.f, t2 = 0.f;
      for (int l = 0; l < lanes; ++l) { t1 += red[0][l * W + ch]; t2 += red[1][l * W + ch]; }
      if (lane0 == 0) {
        ws[row * 2 * c + ch] = t1;          // row = the block's pixel range
        ws[row * 2 * c + c + ch] = t2;
      } else {
        ws[row * 2 * c + ch] += t1;
        ws[row * 2 * c + c + ch] += t2;
      }
    }
    __syncthreads();
  }
}

__device__ __forceinline__ void last_block_finish(int c, const float* ws, float (&red)[2][2048 + 64],
                                                  const BwdFin& fin, const unsigned nblk) {
  // in-launch finalize (cdna_hip_programming.md G16 counter hand-off): every wave drains its
  // partial-row stores, one agent-scope release + ticket; the block drawing the last ticket
  // acquires and sums all rows in a fixed order (deterministic whichever block is last)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  unsigned* flag = reinterpret_cast<unsigned*>(&red[0][0]);
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned t = __hip_atomic_fetch_add(fin.cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned last = (t == nblk - 1) ? 1u : 0u;
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    flag[0] = last;
  }
  __syncthreads();
  if (flag[0] == 0) return;
  __syncthreads();
  const int rows = nblk, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  double* dred = reinterpret_cast<double*>(&red[0][0]);     // [2][8][33] doubles
  for (int cb = 0; cb < c; cb += 32) {
    const int ch = cb + tx;
    double b1[4] = {0, 0, 0, 0}, b2[4] = {0, 0, 0, 0};
    if (ch < c) {
      int r = ty;
      for (; r + 24 < rows; r += 32) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          b1[u] += ws[(long)(r + 8 * u) * 2 * c + ch];
          b2[u] += ws[(long)(r + 8 * u) * 2 * c + c + ch];
        }
      }
      for (; r < rows; r += 8) {
        b1[0] += ws[(long)r * 2 * c + ch];
        b2[0] += ws[(long)r * 2 * c + c + ch];
      }
    }
    dred[(0 * 8 + ty) * 33 + tx] = (b1[0] + b1[1]) + (b1[2] + b1[3]);
    dred[(1 * 8 + ty) * 33 + tx] = (b2[0] + b2[1]) + (b2[2] + b2[3]);
    __syncthreads();
    if (ty == 0 && ch < c) {
      double t1 = 0.0, t2 = 0.0;
      for (int k = 0; k < 8; ++k) { t1 += dred[(0 * 8 + k) * 33 + tx]; t2 += dred[(1 * 8 + k) * 33 + tx]; }
      if (fin.dbeta) fin.dbeta[ch] = (float)t1;
      if (fin.dgamma) fin.dgamma[ch] = (float)t2;
      if (fin.coef) {
        fin.coef[ch] = (float)(t1 / (double)fin.count);
        fin.coef[c + ch] = (float)(t2 / (double)fin.count);
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) __hip_atomic_store(fin.cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// PIPE = false: the serial loop for every c (c % 8 != 0 tails; the host launches PIPE = true)
template <typename T, bool HAS_Z, bool FIN, bool PIPE>
__device__ __forceinline__ void bn_bwd_reduce_body(long npix, int c, const T* z, int z_ld, int z_off, const T* gy,
                                                   int gy_ld, int gy_off, const float* scale, const float* shift,
                                                   const float* mi, int act, float* ws, long ppb, const BwdFin& fin,
                                                   const unsigned bid, const unsigned nblk) {
  __shared__ float red[2][2048 + 64];
  ChanMap m(c);
  const int c0 = m.g * 8, nv = min(8, c - c0);
  float a1[8], a2[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) { a1[i] = 0.f; a2[i] = 0.f; }
  if (m.active) {
    float sc[8], sh[8], mu[8], is[8];
    if (HAS_Z) {
      load_params8(scale, c0, c, sc, 0.f);
      load_params8(shift, c0, c, sh, 0.f);
      load_params8(mi, c0, c, mu, 0.f);
      load_params8(mi + c, c0, c, is, 0.f);
    }
    const long p0 = block_range<BN_REV_RED>(bid, nblk) * ppb, p1 = min(npix, p0 + ppb);
    auto accum = [&](const Raw8<T>& g, const Raw8<T>& zz) {
      float gv[8], zv[8];
      unpack8(g, gv);
      if (HAS_Z) unpack8(zz, zv);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        float da = gv[i], xh = 0.f;
        if (HAS_Z) {
          const float a = zv[i] * sc[i] + sh[i];
          if (act == YMS_ACT_SILU) da = gv[i] * dsilu_f(a);
          xh = (zv[i] - mu[i]) * is[i];
        }
        a1[i] += da;
        a2[i] += da * xh;
      }
    };
    const long step = (long)m.PY * BN_UR;
    if (PIPE && c % 8 == 0) {
      // software-pipelined: the next U pixels' loads are in flight while this U's math runs
      // (2 blocks per CU leave too few waves to hide HBM latency otherwise).  Loads are
      // unconditional -- pixels past the range re-read the last one and are masked out of the
      // sums -- so no branch separates a load from its wait and vmcnt can count.
      auto issue = [&](long b, Raw8<T> (&g)[BN_UR], Raw8<T> (&zz)[BN_UR]) {
#pragma unroll
        for (int u = 0; u < BN_UR; ++u) {
          const long pix = min(b + (long)u * m.PY, p1 - 1);
          load_raw8(gy + pix * gy_ld + gy_off + c0, 8, g[u]);
          if (HAS_Z) load_raw8(z + pix * z_ld + z_off + c0, 8, zz[u]);
        }
      };
      auto consume = [&](long b, const Raw8<T> (&g)[BN_UR], const Raw8<T> (&zz)[BN_UR]) {
#pragma unroll
        for (int u = 0; u < BN_UR; ++u)
          if (b + (long)u * m.PY < p1) accum(g[u], zz[u]);
      };
      long base = p0 + m.py;
      if (base < p1) {
        Raw8<T> ga[BN_UR], za[BN_UR], gb[BN_UR], zb[BN_UR];
        issue(base, ga, za);
        while (true) {
          issue(base + step, gb, zb);
          consume(base, ga, za);
          base += step;
          if (base >= p1) break;
          issue(base + step, ga, za);
          consume(base, gb, zb);
          base += step;
          if (base >= p1) break;
        }
      }
    } else {
      for (long base = p0 + m.py; base < p1; base += step) {
        Raw8<T> gr[BN_UR], zr[BN_UR];
#pragma unroll
        for (int u = 0; u < BN_UR; ++u) {
          const long pix = base + (long)u * m.PY;
          if (pix < p1) {
            load_raw8(gy + pix * gy_ld + gy_off + c0, nv, gr[u]);
            if (HAS_Z) load_raw8(z + pix * z_ld + z_off + c0, nv, zr[u]);
          }
        }
#pragma unroll
        for (int u = 0; u < BN_UR; ++u)
          if (base + (long)u * m.PY < p1) accum(gr[u], zr[u]);
      }
    }
  }
  block_rows_store(m, c, c0, a1, a2, red, ws, block_range<BN_REV_RED>(bid, nblk));
  if constexpr (FIN) last_block_finish(c, ws, red, fin, nblk);
}
template <typename T, bool HAS_Z, bool FIN = false, bool PIPE = true>
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(long npix, int c, const T* z, int z_ld,
                                                            int z_off, const T* gy, int gy_ld, int gy_off,
                                                            const float* scale, const float* shift,
                                                            const float* mi, int act, float* ws, long ppb,
                                                            BwdFin fin = BwdFin{}) {
  bn_bwd_reduce_body<T, HAS_Z, FIN, PIPE>(npix, c, z, z_ld, z_off, gy, gy_ld, gy_off, scale, shift, mi, act, ws, ppb,
                                          fin, blockIdx.x, gridDim.x);
}
// grouped: the BN + act reduce (HAS_Z, separate finalize) ...
template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_reduce_group_kernel(BnGroup<PassJob> grp) {
  unsigned bid, nblk;
  const PassJob& j = grp.job[group_member(grp, bid, nblk)];
  bn_bwd_reduce_body<T, true, false, true>(j.npix, j.c, (const T*)j.z, j.z_ld, j.z_off, (const T*)j.gy, j.gy_ld,
                                           j.gy_off, j.scale, j.shift, j.mi, j.act, j.ws, j.ppb, BwdFin{}, bid, nblk);
}
// ... and the bias reduce with its in-launch finalize (each member its own arrival counter)
struct BiasJob {
  long npix, ppb;
  int c;
  const void* gy; int gy_ld, gy_off;
  float* ws;
  BwdFin fin;
};
template <typename T>
__global__ __launch_bounds__(256) void bias_bwd_group_kernel(BnGroup<BiasJob> grp) {
  unsigned bid, nblk;
  const BiasJob& j = grp.job[group_member(grp, bid, nblk)];
  bn_bwd_reduce_body<T, false, true, true>(j.npix, j.c, (const T*)nullptr, 0, 0, (const T*)j.gy, j.gy_ld, j.gy_off,
                                           nullptr, nullptr, nullptr, YMS_ACT_NONE, j.ws, j.ppb, j.fin, bid, nblk);
}

// 32 channels x TY row lanes per block.  TY = 8 (256 threads) by default: with the weight
// gradients running on the side stream, a 1024-thread block waits for a whole CU to drain,
// which puts that wait on the main stream's critical path.
template <int TY>
__device__ __forceinline__ void bn_bwd_finalize_body(int c, const float* ws, int rows, long count, float* dgamma,
                                                     float* dbeta, float* coef, const unsigned bid) {
  __shared__ double red[2][TY][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int ch = bid * 32 + tx;
  double a1[4] = {0, 0, 0, 0}, a2[4] = {0, 0, 0, 0};
  if (ch < c) {
    int r = ty;
    for (; r + 3 * TY < rows; r += 4 * TY) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        a1[u] += ws[(long)(r + TY * u) * 2 * c + ch];
        a2[u] += ws[(long)(r + TY * u) * 2 * c + c + ch];
      }
    }
    for (; r < rows; r += TY) {
      a1[0] += ws[(long)r * 2 * c + ch];
      a2[0] += ws[(long)r * 2 * c + c + ch];
    }
  }
  red[0][ty][tx] = (a1[0] + a1[1]) + (a1[2] + a1[3]);
  red[1][ty][tx] = (a2[0] + a2[1]) + (a2[2] + a2[3]);
  __syncthreads();
  if (ty == 0 && ch < c) {
    double t1 = 0.0, t2 = 0.0;
    for (int k = 0; k < TY; ++k) { t1 += red[0][k][tx]; t2 += red[1][k][tx]; }
    if (dbeta) dbeta[ch] = (float)t1;
    if (dgamma) dgamma[ch] = (float)t2;
    if (coef) {
      coef[ch] = (float)(t1 / (double)count);
      coef[c + ch] = (float)(t2 / (double)count);
    }
  }
}
template <int TY>
__global__ __launch_bounds__(32 * TY) void bn_bwd_finalize_kernel(int c, const float* ws, int rows, long count,
                                                                  float* dgamma, float* dbeta, float* coef) {
  bn_bwd_finalize_body<TY>(c, ws, rows, count, dgamma, dbeta, coef, blockIdx.x);
}
struct BwdFinJob {
  int c, rows;
  const float* ws;
  long count;
  float *dgamma, *dbeta, *coef;
};
template <int TY>
__global__ __launch_bounds__(32 * TY) void bn_bwd_finalize_group_kernel(BnGroup<BwdFinJob> grp) {
  unsigned bid, nblk;
  const BwdFinJob& j = grp.job[group_member(grp, bid, nblk)];
  bn_bwd_finalize_body<TY>(j.c, j.ws, j.rows, j.count, j.dgamma, j.dbeta, j.coef, bid);
}

// PIPE (the default): software-pipelined like the reduce (c % 8 == 0): the next U pixels' loads (clamped to
// the block's last pixel, masked) are in flight while this U is computed and stored.  Stores stay
// masked: dz may overwrite z in place and gres may accumulate, so a duplicate pixel must not be
// written twice.
template <typename T, bool PIPE>
__device__ __forceinline__ void bn_bwd_apply_body(long npix, int c, const T* z, int z_ld, int z_off, const T* gy,
                                                  int gy_ld, int gy_off, const float* scale, const float* shift,
                                                  const float* mi, const float* coef, int act, T* dz, int dz_ld,
                                                  int dz_off, T* gres, int gres_ld, int gres_off, int gres_acc,
                                                  long ppb, const unsigned bid, const unsigned nblk) {
  ChanMap m(c);
  if (!m.active) return;
  const int c0 = m.g * 8, nv = min(8, c - c0);
  // dz = sc*(da - k0 - (z-mu)*is*k1) = sc*da + A + B*z
  float sc[8], sh[8], A[8], Bz[8];
  {
    float mu[8], is[8], k0[8], k1[8];
    load_params8(scale, c0, c, sc, 0.f);
    load_params8(shift, c0, c, sh, 0.f);
    load_params8(mi, c0, c, mu, 0.f);
    load_params8(mi + c, c0, c, is, 0.f);
    load_params8(coef, c0, c, k0, 0.f);
    load_params8(coef + c, c0, c, k1, 0.f);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      Bz[i] = -sc[i] * k1[i] * is[i];
      A[i] = -sc[i] * k0[i] - Bz[i] * mu[i];
    }
  }
  const long p0 = block_range<BN_REV_APPLY>(bid, nblk) * ppb, p1 = min(npix, p0 + ppb);
  const bool racc = gres && gres_acc;
  auto emit = [&](long pix, const Raw8<T>& g, const Raw8<T>& zz, const Raw8<T>& rres, int valid) {
    float gv[8], zv[8], out[8];
    unpack8(g, gv);
    unpack8(zz, zv);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      float da = gv[i];
      if (act == YMS_ACT_SILU) da *= dsilu_f(zv[i] * sc[i] + sh[i]);
      out[i] = sc[i] * da + A[i] + Bz[i] * zv[i];
    }
    if (gres) {
      float r[8];
      if (gres_acc) {
        unpack8(rres, r);
#pragma unroll
        for (int i = 0; i < 8; ++i) r[i] += gv[i];
        store8(gres + pix * gres_ld + gres_off + c0, valid, r);
      } else {
        store8(gres + pix * gres_ld + gres_off + c0, valid, gv);
      }
    }
    store8(dz + pix * dz_ld + dz_off + c0, valid, out);
  };
  const long step = (long)m.PY * BN_UA;
  if (PIPE && c % 8 == 0) {
    auto issue = [&](long b, Raw8<T> (&g)[BN_UA], Raw8<T> (&zz)[BN_UA], Raw8<T> (&rres)[BN_UA]) {
#pragma unroll
      for (int u = 0; u < BN_UA; ++u) {
        const long pix = min(b + (long)u * m.PY, p1 - 1);
        load_raw8_nt(gy + pix * gy_ld + gy_off + c0, g[u]);     // the last reads of gy and z
        load_raw8_nt(z + pix * z_ld + z_off + c0, zz[u]);
        if (racc) load_raw8(gres + pix * gres_ld + gres_off + c0, 8, rres[u]);
      }
    };
    auto consume = [&](long b, const Raw8<T> (&g)[BN_UA], const Raw8<T> (&zz)[BN_UA], const Raw8<T> (&rres)[BN_UA]) {
#pragma unroll
      for (int u = 0; u < BN_UA; ++u) {
        const long pix = b + (long)u * m.PY;
        if (pix < p1) emit(pix, g[u], zz[u], rres[u], 8);
      }
    };
    long base = p0 + m.py;
    if (base < p1) {
      Raw8<T> ga[BN_UA], za[BN_UA], ra[BN_UA], gb[BN_UA], zb[BN_UA], rb[BN_UA];
      issue(base, ga, za, ra);
      // the next group's loads go out before this group's stores.  Every pixel is loaded and
      // stored by one thread (in-place dz over z is per pixel and per thread); a clamped load of
      // another thread's pixel may see its dz, but that value is masked and never stored
      while (true) {
        issue(base + step, gb, zb, rb);
        consume(base, ga, za, ra);
        base += step;
        if (base >= p1) break;
        issue(base + step, ga, za, ra);
        consume(base, gb, zb, rb);
        base += step;
        if (base >= p1) break;
      }
    }
  } else {
    for (long base = p0 + m.py; base < p1; base += step) {
      Raw8<T> gr[BN_UA], zr[BN_UA], rr[BN_UA];
#pragma unroll
      for (int u = 0; u < BN_UA; ++u) {
        const long pix = base + (long)u * m.PY;
        if (pix < p1) {
          load_raw8(gy + pix * gy_ld + gy_off + c0, nv, gr[u]);
          load_raw8(z + pix * z_ld + z_off + c0, nv, zr[u]);
          if (racc) load_raw8(gres + pix * gres_ld + gres_off + c0, nv, rr[u]);
        }
      }
#pragma unroll
      for (int u = 0; u < BN_UA; ++u) {
        const long pix = base + (long)u * m.PY;
        if (pix < p1) emit(pix, gr[u], zr[u], rr[u], nv);
      }
    }
  }
}
template <typename T, bool PIPE = false>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(long npix, int c, const T* z, int z_ld, int z_off,
                                                           const T* gy, int gy_ld, int gy_off, const float* scale,
                                                           const float* shift, const float* mi,
                                                           const float* coef, int act, T* dz, int dz_ld,
                                                           int dz_off, T* gres, int gres_ld, int gres_off,
                                                           int gres_acc, long ppb) {
  bn_bwd_apply_body<T, PIPE>(npix, c, z, z_ld, z_off, gy, gy_ld, gy_off, scale, shift, mi, coef, act, dz, dz_ld, dz_off,
                             gres, gres_ld, gres_off, gres_acc, ppb, blockIdx.x, gridDim.x);
}
template <typename T, bool PIPE>
__global__ __launch_bounds__(256) void bn_bwd_apply_group_kernel(BnGroup<PassJob> grp) {
  unsigned bid, nblk;
  const PassJob& j = grp.job[group_member(grp, bid, nblk)];
  bn_bwd_apply_body<T, PIPE>(j.npix, j.c, (const T*)j.z, j.z_ld, j.z_off, (const T*)j.gy, j.gy_ld, j.gy_off, j.scale,
                             j.shift, j.mi, j.coef, j.act, (T*)j.out, j.out_ld, j.out_off, (T*)j.res, j.res_ld,
                             j.res_off, j.res_acc, j.ppb, bid, nblk);
}

// ------------------------------------------------------------------------------------------
// BN with RUNNING statistics (a BatchNorm2d in eval mode inside a training step) + act, backward in
// ONE pass.  The normalisation is a fixed per-channel affine map, so dz needs no batch sums:
//   da = gy * act'(z*scale + shift),  dz = scale * da  (over z, in place, or elsewhere),
//   gres = gy or gres += gy,  and, SUMS, dbeta = sum da, dgamma = sum da * (z - running_mean) * invstd
// through the partial rows and the in-launch finalize of the reduce above.  gy and z are read once
// (two reads + one write per element, against the three passes' four reads + one write).
// The loop is the apply pass's: every pixel is loaded, summed and stored by ONE thread, the next
// group's loads go out before this group's stores, and a clamped duplicate (another thread's pixel,
// perhaps already overwritten by its dz) is masked out of the sums and the stores alike.
// ------------------------------------------------------------------------------------------
template <typename T, bool SUMS>
__global__ __launch_bounds__(256) void bn_frozen_bwd_kernel(const PassJob j, const BwdFin fin) {
  ChanMap m(j.c);
  const int c = j.c, c0 = m.g * 8, nv = min(8, c - c0);
  const T *z = (const T*)j.z, *gy = (const T*)j.gy;
  T *dz = (T*)j.out, *gres = (T*)j.res;
  float a1[8], a2[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) { a1[i] = 0.f; a2[i] = 0.f; }
  if (m.active) {
    float sc[8], sh[8], mu[8], is[8];
    load_params8(j.scale, c0, c, sc, 0.f);
    load_params8(j.shift, c0, c, sh, 0.f);
    if (SUMS) {
      load_params8(j.mi, c0, c, mu, 0.f);
      load_params8(j.mi + c, c0, c, is, 0.f);
    }
    const long p0 = (long)blockIdx.x * j.ppb, p1 = min(j.npix, p0 + j.ppb);
    const int act = j.act;
    const bool racc = gres && j.res_acc;
    auto emit = [&](long pix, const Raw8<T>& g, const Raw8<T>& zz, const Raw8<T>& rres, int valid) {
      float gv[8], zv[8], out[8];
      unpack8(g, gv);
      unpack8(zz, zv);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        float da = gv[i];
        if (act == YMS_ACT_SILU) da *= dsilu_f(zv[i] * sc[i] + sh[i]);
        out[i] = sc[i] * da;
        if (SUMS) {
          a1[i] += da;
          a2[i] += da * ((zv[i] - mu[i]) * is[i]);
        }
      }
      if (gres) {
        if (racc) {
          float r[8];
          unpack8(rres, r);
#pragma unroll
          for (int i = 0; i < 8; ++i) r[i] += gv[i];
          store8(gres + pix * j.res_ld + j.res_off + c0, valid, r);
        } else {
          store8(gres + pix * j.res_ld + j.res_off + c0, valid, gv);
        }
      }
      store8(dz + pix * j.out_ld + j.out_off + c0, valid, out);
    };
    const long step = (long)m.PY * BN_UA;
    if (c % 8 == 0) {
      auto issue = [&](long b, Raw8<T> (&g)[BN_UA], Raw8<T> (&zz)[BN_UA], Raw8<T> (&rres)[BN_UA]) {
#pragma unroll
        for (int u = 0; u < BN_UA; ++u) {
          const long pix = min(b + (long)u * m.PY, p1 - 1);
          load_raw8(gy + pix * j.gy_ld + j.gy_off + c0, 8, g[u]);
          load_raw8(z + pix * j.z_ld + j.z_off + c0, 8, zz[u]);
          if (racc) load_raw8(gres + pix * j.res_ld + j.res_off + c0, 8, rres[u]);
        }
      };
      auto consume = [&](long b, const Raw8<T> (&g)[BN_UA], const Raw8<T> (&zz)[BN_UA], const Raw8<T> (&rres)[BN_UA]) {
#pragma unroll
        for (int u = 0; u < BN_UA; ++u) {
          const long pix = b + (long)u * m.PY;
          if (pix < p1) emit(pix, g[u], zz[u], rres[u], 8);
        }
      };
      long base = p0 + m.py;
      if (base < p1) {
        Raw8<T> ga[BN_UA], za[BN_UA], ra[BN_UA], gb[BN_UA], zb[BN_UA], rb[BN_UA];
        issue(base, ga, za, ra);
        while (true) {
          issue(base + step, gb, zb, rb);
          consume(base, ga, za, ra);
          base += step;
          if (base >= p1) break;
          issue(base + step, ga, za, ra);
          consume(base, gb, zb, rb);
          base += step;
          if (base >= p1) break;
        }
      }
    } else {
      for (long base = p0 + m.py; base < p1; base += step) {
        Raw8<T> gr[BN_UA], zr[BN_UA], rr[BN_UA];
#pragma unroll
        for (int u = 0; u < BN_UA; ++u) {
          const long pix = base + (long)u * m.PY;
          if (pix < p1) {
            load_raw8(gy + pix * j.gy_ld + j.gy_off + c0, nv, gr[u]);
            load_raw8(z + pix * j.z_ld + j.z_off + c0, nv, zr[u]);
            if (racc) load_raw8(gres + pix * j.res_ld + j.res_off + c0, nv, rr[u]);
          }
        }
#pragma unroll
        for (int u = 0; u < BN_UA; ++u) {
          const long pix = base + (long)u * m.PY;
          if (pix < p1) emit(pix, gr[u], zr[u], rr[u], nv);
        }
      }
    }
  }
  if constexpr (SUMS) {
    __shared__ float red[2][2048 + 64];
    block_rows_store(m, c, c0, a1, a2, red, j.ws, (long)blockIdx.x);
    last_block_finish(c, j.ws, red, fin, gridDim.x);
  }
}

// ------------------------------------------------------------------------------------------
// SPPF pools: slot k = clipped (4k+1)x(4k+1) window max of slot 0 (== k chained MaxPool5).
// ------------------------------------------------------------------------------------------
// One MaxPool2d(5, 1, 2) of the SPPF chain: slot `out` = pool5(slot `in`) (-inf padding).
// For the planes the one-launch kernels below do not take (yms_sppf_fused_fits: fp32, more than 585
// positions), the chain p1 = pool(x), p2 = pool(p1), p3 = pool(p2) runs as three launches (75 loads per
// output group instead of the 169 of a direct 13x13 window); max is exact and a NaN in the window
// wins (torch's `val > max || isnan(val)`), so the result is bit-identical to the reference's chained
// pools.
template <typename T>
__global__ __launch_bounds__(256) void pool5_fwd_kernel(int n, int h, int w, int c, T* buf, int ld, int in_off,
                                                        int out_off) {
  const int G = c >> 3;
  const uint32_t total = (uint32_t)n * h * w * G;
  for (uint32_t t = blockIdx.x * 256u + threadIdx.x; t < total; t += gridDim.x * 256u) {
    const uint32_t g = t % G, pix = t / G;
    const uint32_t x = pix % w, r = pix / w;
    const uint32_t y = r % h, b = r / h;
    float m[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) m[i] = -INFINITY;
    const int y0 = max((int)y - 2, 0), y1 = min((int)y + 2, h - 1);
    const int x0 = max((int)x - 2, 0), x1 = min((int)x + 2, w - 1);
    for (int yy = y0; yy <= y1; ++yy) {
      const T* row = buf + ((long)(b * h + yy) * w) * ld + in_off + g * 8;
      for (int xx = x0; xx <= x1; ++xx) {
        float v[8];
        Vec8<T>::load(row + (long)xx * ld, v);
#pragma unroll
        for (int i = 0; i < 8; ++i) m[i] = (v[i] > m[i] || v[i] != v[i]) ? v[i] : m[i];   // NaN propagates (torch)
      }
    }
    Vec8<T>::store(buf + (long)pix * ld + out_off + g * 8, m);
  }
}

// argmax of a 5x5 (pad 2, -inf) window over input slot `in`, PyTorch scan order, first max.
template <typename T>
__global__ void pool5_argmax_kernel(int n, int h, int w, int c, const T* buf, int ld, int in_off,
                                    uint8_t* arg) {
  const int G = (c + 7) >> 3;
  const uint32_t total = (uint32_t)n * h * w * G;
  for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += gridDim.x * blockDim.x) {
    const int g = (int)(t % G);
    uint32_t r = t / G;
    const int x = (int)(r % w);
    r /= w;
    const int y = (int)(r % h);
    const int b = (int)(r / h);
    const int c0 = g * 8, nv = min(8, c - c0);
    float best[8];
    uint8_t idx[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) { best[i] = -INFINITY; idx[i] = 255; }
    for (int ky = 0; ky < 5; ++ky) {
      const int yy = y - 2 + ky;
      if (yy < 0 || yy >= h) continue;
      for (int kx = 0; kx < 5; ++kx) {
        const int xx = x - 2 + kx;
        if (xx < 0 || xx >= w) continue;
        float v[8];
        load8(buf + (((long)b * h + yy) * w + xx) * ld + in_off + c0, nv, v);
#pragma unroll
        for (int i = 0; i < 8; ++i)
          if (idx[i] == 255 || v[i] > best[i] || v[i] != v[i]) {  // (val > maxval) || isnan(val)
            best[i] = v[i];
            idx[i] = (uint8_t)(ky * 5 + kx);
          }
      }
    }
    uint8_t* a = arg + ((((long)b * h + y) * w + x) * G + g) * 8;
#pragma unroll
    for (int i = 0; i < 8; ++i) a[i] = idx[i];
  }
}

// g[in slot] += sum over the 25 outputs o whose argmax points at this position of g[out slot]
template <typename T>
__global__ void pool5_gather_kernel(int n, int h, int w, int c, const uint8_t* arg, T* g, int ld,
                                    int in_off, int out_off) {
  const int G = (c + 7) >> 3;
  const uint32_t total = (uint32_t)n * h * w * G;
  for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += gridDim.x * blockDim.x) {
    const int gg = (int)(t % G);
    uint32_t r = t / G;
    const int x = (int)(r % w);
    r /= w;
    const int y = (int)(r % h);
    const int b = (int)(r / h);
    const int c0 = gg * 8, nv = min(8, c - c0);
    float acc[8];
    load8(g + (((long)b * h + y) * w + x) * ld + in_off + c0, nv, acc);
    // output o = (y - ky + 2, x - kx + 2) sees this input at window offset (ky, kx)
    for (int ky = 0; ky < 5; ++ky) {
      const int oy = y - ky + 2;
      if (oy < 0 || oy >= h) continue;
      for (int kx = 0; kx < 5; ++kx) {
        const int ox = x - kx + 2;
        if (ox < 0 || ox >= w) continue;
        const long o = ((long)b * h + oy) * w + ox;
        const uint8_t* a = arg + (o * G + gg) * 8;
        const uint2 av = *reinterpret_cast<const uint2*>(a);
        const uint8_t want = (uint8_t)(ky * 5 + kx);
        float gv[8];
        load8(g + o * ld + out_off + c0, nv, gv);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const uint8_t ai = (uint8_t)(((i < 4 ? av.x : av.y) >> (8 * (i & 3))) & 0xff);
          if (ai == want) acc[i] += gv[i];
        }
      }
    }
    store8(g + (((long)b * h + y) * w + x) * ld + in_off + c0, nv, acc);
  }
}

// ------------------------------------------------------------------------------------------
// SPPF chain in one launch (16-bit types, planes that fit the LDS budget below)
// ------------------------------------------------------------------------------------------
// One block owns one (image, 8-channel chunk): its h x w plane of 16-B items lives in LDS for
// the whole chain, so the intermediate slots never come back from memory and nothing is shared
// between blocks.  Each 5x5 pool runs as a row pass and a column pass (10 taps instead of 25).
// That is the 25-tap scan of pool5_fwd_kernel / pool5_argmax_kernel bit for bit: every in-bounds
// row of a clipped window has the same in-bounds columns, the row pass keeps the first maximum
// (or the last NaN) of its row, and the column pass, replacing on `v > m || v != v` over rows in
// order, keeps the first row holding the maximum (or the last holding a NaN) -- the lexicographic
// (row, column) choice of the 2-D scan, zero sign and argmax included.
//
// Logical block l = image * G + chunk, chunks fastest, in dw_block's order (dwconv.hip): the grid
// is padded to a multiple of 8 and block i, which runs on XCD i % 8, takes logical block
// (i % 8) * (grid / 8) + i / 8.  The eight chunk-blocks that share a pixel's 128-B line are then
// consecutive blocks of one XCD and find the rest of each line in its L2.
constexpr int SPPF_NP = 3;                    // plane positions per thread (256 threads)
constexpr int SPPF_BWD_BPP = 56;              // backward LDS bytes per position (see the kernel)
constexpr int SPPF_LDS_MAX = 32 * 1024;       // per block: two blocks fit beside a 64-KB weight-gradient block

template <typename T>
__device__ __forceinline__ u32x4 sppf_pack(const float (&v)[8]) {
  T t[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) t[i] = (T)v[i];
  u32x4 r;
  __builtin_memcpy(&r, t, sizeof(r));
  return r;
}
template <typename T>
__device__ __forceinline__ void sppf_unpack(const u32x4& r, float (&v)[8]) {
  Raw8<T> q;
  q.v[0] = r;
  unpack8<T>(q, v);
}
__device__ __forceinline__ bool sppf_block(int nlog, int G, int& b, int& g) {
  const int l = (int)((blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3));
  if (l >= nlog) return false;
  g = l % G;
  b = l / G;
  return true;
}

template <typename T>
__global__ __launch_bounds__(256) void sppf_chain_fwd_kernel(int nlog, int h, int w, int c, T* buf, int ld, int off) {
  static_assert(sizeof(T) == 2, "16-bit planes");
  extern __shared__ u32x4 sppf_lds[];
  int b, g;
  if (!sppf_block(nlog, c >> 3, b, g)) return;
  const int P = h * w;
  u32x4* X = sppf_lds;        // slot k - 1, then slot k
  u32x4* R = sppf_lds + P;    // row maxima
  T* base = buf + (long)b * P * ld + off + g * 8;
  int py[SPPF_NP], px[SPPF_NP];
#pragma unroll
  for (int i = 0; i < SPPF_NP; ++i) {
    const int p = threadIdx.x + 256 * i;
    py[i] = p / w;
    px[i] = p - py[i] * w;
    if (p < P) X[p] = *reinterpret_cast<const u32x4*>(base + (long)p * ld);
  }
  __syncthreads();
  for (int k = 1; k <= 3; ++k) {
#pragma unroll
    for (int i = 0; i < SPPF_NP; ++i) {
      const int p = threadIdx.x + 256 * i;
      if (p >= P) continue;
      float m[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) m[j] = -INFINITY;
      const int x0 = max(px[i] - 2, 0), x1 = min(px[i] + 2, w - 1);
      for (int q = p - px[i] + x0; q <= p - px[i] + x1; ++q) {
        float v[8];
        sppf_unpack<T>(X[q], v);
#pragma unroll
        for (int j = 0; j < 8; ++j) m[j] = (v[j] > m[j] || v[j] != v[j]) ? v[j] : m[j];
      }
      R[p] = sppf_pack<T>(m);
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < SPPF_NP; ++i) {
      const int p = threadIdx.x + 256 * i;
      if (p >= P) continue;
      float m[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) m[j] = -INFINITY;
      const int y0 = max(py[i] - 2, 0), y1 = min(py[i] + 2, h - 1);
      for (int yy = y0; yy <= y1; ++yy) {
        float v[8];
        sppf_unpack<T>(R[yy * w + px[i]], v);
#pragma unroll
        for (int j = 0; j < 8; ++j) m[j] = (v[j] > m[j] || v[j] != v[j]) ? v[j] : m[j];
      }
      const u32x4 r = sppf_pack<T>(m);
      X[p] = r;     // the row pass was the last reader of slot k - 1
      *reinterpret_cast<u32x4*>(base + (long)p * ld + k * c) = r;
    }
    __syncthreads();
  }
}

// Backward of the chain.  LDS per position: V (16 B: the value plane of slot k - 1; once the row
// pass has read it, its first 8 B per position hold the argmax bytes), two 16-B planes that
// alternate between "gradient of slot k" and "row maxima, then the rounded gradient of slot
// k - 1", and 8 B of row argmax columns: 56 B.  The next stage's value plane and the gradient
// its positions start from (slot k - 2) wait in registers, loaded before the gather that hides them.
template <typename T>
__global__ __launch_bounds__(256) void sppf_chain_bwd_kernel(int nlog, int h, int w, int c, const T* buf, int ld,
                                                             int off, T* gbuf, int gld, int goff) {
  static_assert(sizeof(T) == 2, "16-bit planes");
  extern __shared__ u32x4 sppf_lds[];
  int b, g;
  if (!sppf_block(nlog, c >> 3, b, g)) return;
  const int P = h * w;
  u32x4* V = sppf_lds;
  uint2* A = reinterpret_cast<uint2*>(sppf_lds);
  u32x4* GI = sppf_lds + P;          // gradient of slot k
  u32x4* GO = sppf_lds + 2 * P;      // row maxima, then gradient of slot k - 1
  uint2* RK = reinterpret_cast<uint2*>(sppf_lds + 3 * P);
  const T* vbase = buf + (long)b * P * ld + off + g * 8;
  T* gbase = gbuf + (long)b * P * gld + goff + g * 8;
  u32x4 vreg[SPPF_NP], greg[SPPF_NP];
#pragma unroll
  for (int i = 0; i < SPPF_NP; ++i) {
    const int p = threadIdx.x + 256 * i;
    vreg[i] = greg[i] = u32x4{0u, 0u, 0u, 0u};
    if (p < P) {
      vreg[i] = *reinterpret_cast<const u32x4*>(vbase + (long)p * ld + 2 * c);
      greg[i] = *reinterpret_cast<const u32x4*>(gbase + (long)p * gld + 2 * c);
      GI[p] = *reinterpret_cast<const u32x4*>(gbase + (long)p * gld + 3 * c);
    }
  }
  for (int k = 3; k >= 1; --k) {
#pragma unroll
    for (int i = 0; i < SPPF_NP; ++i) {
      const int p = threadIdx.x + 256 * i;
      if (p < P) V[p] = vreg[i];     // the previous gather's reads of A ended at its closing barrier
    }
    __syncthreads();
    // row pass: first maximum (last NaN) of the in-bounds columns of each row window, and its kx
#pragma unroll 1
    for (int p = threadIdx.x; p < P; p += 256) {
      const int px = p % w;
      const int kx0 = max(2 - px, 0), kx1 = min(w + 1 - px, 4);
      float best[8];
      uint32_t idx[8];
      sppf_unpack<T>(V[p - 2 + kx0], best);
#pragma unroll
      for (int j = 0; j < 8; ++j) idx[j] = (uint32_t)kx0;
      for (int kx = kx0 + 1; kx <= kx1; ++kx) {
        float v[8];
        sppf_unpack<T>(V[p - 2 + kx], v);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const bool t = v[j] > best[j] || v[j] != v[j];
          best[j] = t ? v[j] : best[j];
          idx[j] = t ? (uint32_t)kx : idx[j];
        }
      }
      GO[p] = sppf_pack<T>(best);
      RK[p] = make_uint2(idx[0] | idx[1] << 8 | idx[2] << 16 | idx[3] << 24,
                         idx[4] | idx[5] << 8 | idx[6] << 16 | idx[7] << 24);
    }
    __syncthreads();
    // column pass over the row results: the window's argmax byte ky * 5 + kx
#pragma unroll 1
    for (int p = threadIdx.x; p < P; p += 256) {
      const int py = p / w;
      const int ky0 = max(2 - py, 0), ky1 = min(h + 1 - py, 4);
      float best[8];
      uint32_t idx[8];     // the word of candidate bytes that holds channel j's
      {
        const int q = p + (ky0 - 2) * w;
        sppf_unpack<T>(GO[q], best);
        const uint2 rk = RK[q];
        const uint32_t a = 5u * ky0 * 0x01010101u;
#pragma unroll
        for (int j = 0; j < 8; ++j) idx[j] = (j < 4 ? rk.x : rk.y) + a;
      }
      for (int ky = ky0 + 1; ky <= ky1; ++ky) {
        const int q = p + (ky - 2) * w;
        float v[8];
        sppf_unpack<T>(GO[q], v);
        const uint2 rk = RK[q];
        const uint32_t a = 5u * ky * 0x01010101u;
        const uint32_t cx = rk.x + a, cy = rk.y + a;     // bytes < 25: no carry between them
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const bool t = v[j] > best[j] || v[j] != v[j];
          best[j] = t ? v[j] : best[j];
          idx[j] = t ? (j < 4 ? cx : cy) : idx[j];
        }
      }
      uint2 a = make_uint2(0u, 0u);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        a.x |= idx[j] & (0xffu << (8 * j));
        a.y |= idx[4 + j] & (0xffu << (8 * j));
      }
      A[p] = a;      // V's space: the row pass was its last reader
    }
    __syncthreads();
    // the gradient each position starts from takes the row maxima's place (read no more); then the
    // next stage's value plane and starting gradient go in flight over the gather
#pragma unroll
    for (int i = 0; i < SPPF_NP; ++i) {
      const int p = threadIdx.x + 256 * i;
      if (p < P) GO[p] = greg[i];
    }
    if (k > 1) {
#pragma unroll
      for (int i = 0; i < SPPF_NP; ++i) {
        const int p = threadIdx.x + 256 * i;
        if (p < P) {
          vreg[i] = *reinterpret_cast<const u32x4*>(vbase + (long)p * ld + (k - 2) * c);
          greg[i] = *reinterpret_cast<const u32x4*>(gbase + (long)p * gld + (k - 2) * c);
        }
      }
    }
    // gather: g[slot k - 1] + the gradients of the outputs whose argmax is this position, in
    // pool5_gather_kernel's (ky, kx) order, fp32, rounded once
#pragma unroll 1
    for (int p = threadIdx.x; p < P; p += 256) {
      const int py = p / w, px = p - py * w;
      float acc[8];
      sppf_unpack<T>(GO[p], acc);     // this thread's own write
      // output (y - ky + 2, x - kx + 2) sees this input at window offset (ky, kx)
      const int ky0 = max(py + 3 - h, 0), ky1 = min(py + 2, 4);
      const int kx0 = max(px + 3 - w, 0), kx1 = min(px + 2, 4);
      for (int ky = ky0; ky <= ky1; ++ky) {
        for (int kx = kx0; kx <= kx1; ++kx) {
          const int o = p + (2 - ky) * w + 2 - kx;
          const uint2 av = A[o];
          float gv[8];
          sppf_unpack<T>(GI[o], gv);
          const uint32_t want = (uint32_t)(ky * 5 + kx);
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const uint32_t aj = ((j < 4 ? av.x : av.y) >> (8 * (j & 3))) & 0xffu;
            if (aj == want) acc[j] += gv[j];
          }
        }
      }
      const u32x4 r = sppf_pack<T>(acc);
      *reinterpret_cast<u32x4*>(gbase + (long)p * gld + (k - 1) * c) = r;
      GO[p] = r;     // the next stage's incoming gradient
    }
    __syncthreads();
    u32x4* t = GI;
    GI = GO;
    GO = t;
  }
}


// ------------------------------------------------------------------------------------------
// nearest x2 upsample
// ------------------------------------------------------------------------------------------
template <typename T>
__global__ void upsample_fwd_kernel(int n, int h, int w, int c, const T* x, int x_ld, int x_off,
                                    T* y, int y_ld, int y_off) {
  const int G = (c + 7) >> 3;
  const int H2 = 2 * h, W2 = 2 * w;
  const long total = (long)n * H2 * W2 * G;
  for (long t = blockIdx.x * (long)blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
    const int g = (int)(t % G);
    long r = t / G;
    const int X = (int)(r % W2);
    r /= W2;
    const int Y = (int)(r % H2);
    const int b = (int)(r / H2);
    const int c0 = g * 8, nv = min(8, c - c0);
    float v[8];
    load8(x + (((long)b * h + (Y >> 1)) * w + (X >> 1)) * x_ld + x_off + c0, nv, v);
    store8(y + (((long)b * H2 + Y) * W2 + X) * y_ld + y_off + c0, nv, v);
  }
}

template <typename T>
__global__ void upsample_bwd_kernel(int n, int h, int w, int c, const T* gy, int gy_ld, int gy_off,
                                    T* gx, int gx_ld, int gx_off, int accumulate) {
  const int G = (c + 7) >> 3;
  const int W2 = 2 * w;
  const long total = (long)n * h * w * G;
  for (long t = blockIdx.x * (long)blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
    const int g = (int)(t % G);
    long r = t / G;
    const int x = (int)(r % w);
    r /= w;
    const int y = (int)(r % h);
    const int b = (int)(r / h);
    const int c0 = g * 8, nv = min(8, c - c0);
    float s[8];
    T* dst = gx + (((long)b * h + y) * w + x) * gx_ld + gx_off + c0;
    if (accumulate) load8(dst, nv, s);
    else {
#pragma unroll
      for (int i = 0; i < 8; ++i) s[i] = 0.f;
    }
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      float v[8];
      const int Y = 2 * y + (d >> 1), X = 2 * x + (d & 1);
      load8(gy + (((long)b * 2 * h + Y) * W2 + X) * gy_ld + gy_off + c0, nv, v);
#pragma unroll
      for (int i = 0; i < 8; ++i) s[i] += v[i];
    }
    store8(dst, nv, s);
  }
}

// ------------------------------------------------------------------------------------------
// layout / cast
// ------------------------------------------------------------------------------------------
template <typename T>
__global__ void pack_input_kernel(int n, int c, int h, int w, const float* x, T* y, int ld) {
  const long npix = (long)n * h * w;
  const long hw = (long)h * w;
  for (long t = blockIdx.x * (long)blockDim.x + threadIdx.x; t < npix; t += (long)gridDim.x * blockDim.x) {
    const long b = t / hw, s = t - b * hw;
    for (int c0 = 0; c0 < ld; c0 += 8) {
      float v[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = (c0 + i < c) ? x[(b * c + c0 + i) * hw + s] : 0.0f;
      Vec8<T>::store(y + t * ld + c0, v);
    }
  }
}

// NHWC view -> NCHW contiguous, 64x64 (pixel x channel) tiles through LDS.
template <typename TI, typename TO>
__global__ void nhwc_to_nchw_kernel(int n, long hw, int c, const TI* x, int ld, int off, TO* y) {
  __shared__ float tile[64][65];
  const long pt = (long)blockIdx.x * 64;
  const int ct = blockIdx.y * 64;
  const int b = blockIdx.z;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int r = ty; r < 64; r += 4) {
    const long p = pt + r;
    const int ch = ct + tx;
    tile[r][tx] = (p < hw && ch < c) ? (float)x[((long)b * hw + p) * ld + off + ch] : 0.f;
  }
  __syncthreads();
  for (int r = ty; r < 64; r += 4) {
    const int ch = ct + r;
    const long p = pt + tx;
    if (p < hw && ch < c) y[((long)b * c + ch) * hw + p] = (TO)tile[tx][r];
  }
}

template <typename TI, typename TO>
__global__ void nchw_to_nhwc_kernel(int n, long hw, int c, const TI* x, TO* y, int ld, int off,
                                    int accumulate) {
  __shared__ float tile[64][65];
  const long pt = (long)blockIdx.x * 64;
  const int ct = blockIdx.y * 64;
  const int b = blockIdx.z;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int r = ty; r < 64; r += 4) {
    const int ch = ct + r;
    const long p = pt + tx;
    tile[r][tx] = (p < hw && ch < c) ? (float)x[((long)b * c + ch) * hw + p] : 0.f;
  }
  __syncthreads();
  for (int r = ty; r < 64; r += 4) {
    const long p = pt + r;
    const int ch = ct + tx;
    if (p < hw && ch < c) {
      TO* d = y + ((long)b * hw + p) * ld + off + ch;
      float v = tile[tx][r];
      if (accumulate) v += (float)*d;
      *d = (TO)v;
    }
  }
}

template <typename TI, typename TO>
__global__ void cast_kernel(long count, const TI* x, TO* y) {
  for (long t = blockIdx.x * (long)blockDim.x + threadIdx.x; t < count; t += (long)gridDim.x * blockDim.x)
    y[t] = (TO)(float)x[t];
}

}  // namespace yms

using namespace yms;

#define YMS_DT_DISPATCH(dt, T, ...)                 \
  do {                                              \
    if ((dt) == YMS_BF16) { typedef bf16 T; __VA_ARGS__; } \
    else if ((dt) == YMS_F16) { typedef f16 T; __VA_ARGS__; } \
    else if ((dt) == YMS_F32) { typedef float T; __VA_ARGS__; } \
    else return YMS_ERR_INVALID;                    \
  } while (0)

static bool vok(int ld, int off, int c) { return c > 0 && ld % 8 == 0 && off % 8 == 0 && off + c <= ld; }

extern "C" {

yms_status yms_bn_fold(int c, const float* gamma, const float* beta, const float* rmean,
                       const float* rvar, float eps, float* scale, float* shift, void* stream) {
  if (c <= 0 || !scale || !shift) return YMS_ERR_INVALID;
  if (gamma && (!beta || !rmean || !rvar)) return YMS_ERR_INVALID;
  hipLaunchKernelGGL(bn_fold_kernel, dim3(cdiv(c, 256)), dim3(256), 0, (hipStream_t)stream, c, gamma,
                     beta, rmean, rvar, eps, scale, shift);
  return launch_status();
}

}  // extern "C"

// ---- the BN / bias passes ---------------------------------------------------------------------
// Each pass is described ONCE, over its public job record (include/yms.h): check (validation), groupable
// (does the grouped kernel serve this job), blocks and dev (block count and device-side job, from one
// pixels-per-block formula), launch_solo and launch_group.  run_pass runs a pass over n jobs; a solo
// entry point is a job literal and run_pass with n = 1.
static unsigned pix_blocks(long npix, long ppb) { return (unsigned)((npix + ppb - 1) / ppb); }

static PassJob pass_job(const yms_bn_pass_job& j, long ppb) {
  return PassJob{j.npix, ppb, j.c, j.act, j.z, j.z_ld, j.z_off, j.gy, j.gy_ld, j.gy_off, j.scale, j.shift,
                 j.mean_invstd, j.coef, j.out, j.out_ld, j.out_off, j.res, j.res_ld, j.res_off, j.res_acc, j.ws};
}

// The jobs the grouped kernel serves go out BN_GROUP_MAX per launch, each member with its solo launch's
// block count and per-block ranges; a job alone, or one the grouped kernel does not serve, takes the
// solo launch, in job order after the grouped launches.  Every job is checked before the first launch.
template <typename P>
static yms_status run_pass(int dtype, int njobs, const typename P::Job* jobs, void* stream) {
  if (njobs < 0 || (njobs > 0 && !jobs)) return YMS_ERR_INVALID;
  hipStream_t st = (hipStream_t)stream;
  if (njobs == 1) {                           // the solo entry points: no partition, nothing allocated
    const yms_status e = P::check(jobs[0]);
    return e ? e : P::launch_solo(dtype, jobs[0], st);
  }
  std::vector<int> idx;
  for (int i = 0; i < njobs; ++i) {
    if (yms_status e = P::check(jobs[i])) return e;
    if (P::groupable(jobs[i])) idx.push_back(i);
  }
  std::vector<char> grouped(njobs, 0);
  if (idx.size() >= 2) {
    for (size_t i = 0; i < idx.size(); i += BN_GROUP_MAX) {
      const int n = (int)std::min<size_t>(BN_GROUP_MAX, idx.size() - i);
      if (n < 2) break;                      // a lone remainder: solo
      BnGroup<typename P::Dev> g{};
      g.n = n;
      for (int k = 0; k < n; ++k) {
        const typename P::Job& j = jobs[idx[i + k]];
        g.job[k] = P::dev(j);
        g.first[k + 1] = g.first[k] + P::blocks(j);
        grouped[idx[i + k]] = 1;
      }
      if (yms_status e = P::launch_group(dtype, g, g.first[n], st)) return e;
      if (yms_status e = launch_status()) return e;
    }
  }
  for (int i = 0; i < njobs; ++i)
    if (!grouped[i])
      if (yms_status e = P::launch_solo(dtype, jobs[i], st)) return e;
  return YMS_OK;
}

struct FinalizePass {                        // forward: statistics rows -> mean / invstd, scale / shift, running stats
  using Job = yms_bn_finalize_job;
  using Dev = FinJob;
  static yms_status check(const Job& j) {
    if (j.c <= 0 || !j.stats || j.rows <= 0 || j.count <= 0 || !j.gamma || !j.beta || !j.mean_invstd || !j.scale ||
        !j.shift)
      return YMS_ERR_INVALID;
    return j.stats_ld < j.c || j.mi_ld < j.c ? YMS_ERR_INVALID : YMS_OK;
  }
  static bool groupable(const Job& j) { return j.rows <= 1024; }   // long tables: launch_solo's pre-reduction
  static unsigned blocks(const Job& j) { return (unsigned)cdiv(j.c, 8); }
  static Dev dev(const Job& j) {
    return FinJob{j.c, j.rows, j.stats_ld, j.mi_ld, j.stats, j.count, j.gamma, j.beta, j.rmean, j.rvar,
                  j.momentum, j.eps, j.mean_invstd, j.scale, j.shift};
  }
  static yms_status launch_solo(int, const Job& j, hipStream_t st) {
    int rs = 1, nrows = j.rows;
    if (j.rows > 1024) {   // long tables: pre-reduce in parallel (in place), then finalize the partial rows
      const int S = std::min(256, cdiv(j.rows, 64));
      rs = cdiv(j.rows, S);
      nrows = cdiv(j.rows, rs);
      hipLaunchKernelGGL(bn_stats_partial_kernel, dim3(cdiv(j.c, 64), nrows), dim3(256), 0, st, j.c, j.stats, j.rows,
                         j.stats_ld, rs);
    }
    if (rs == 1) {
      hipLaunchKernelGGL(bn_finalize_small_kernel, dim3(blocks(j)), dim3(256), 0, st, j.c, (const float*)j.stats,
                         j.rows, j.stats_ld, j.count, j.gamma, j.beta, j.rmean, j.rvar, j.momentum, j.eps,
                         j.mean_invstd, j.mi_ld, j.scale, j.shift);
      return launch_status();
    }
    hipLaunchKernelGGL(bn_finalize_kernel, dim3(cdiv(j.c, FIN_CW)), dim3(1024), 0, st, j.c, (const float*)j.stats,
                       nrows, j.stats_ld, rs, j.rows, j.count, j.gamma, j.beta, j.rmean, j.rvar, j.momentum, j.eps,
                       j.mean_invstd, j.mi_ld, j.scale, j.shift);
    return launch_status();
  }
  static yms_status launch_group(int, const BnGroup<Dev>& g, unsigned nb, hipStream_t st) {
    hipLaunchKernelGGL(bn_finalize_small_group_kernel, dim3(nb), dim3(256), 0, st, g);
    return YMS_OK;
  }
};

// pixels per block for the channel-stationary kernels: about four U-pixel iterations per
// thread (amortises the per-channel parameter loads; measured best of 1/2/4/8), at most 8192
// blocks
static long elem_ppb(long npix, int c, int iters = 4) {
  const long py = 256 / ((c + 7) / 8);
  long blocks = std::min<long>(std::max<long>(cdiv(npix, py * BN_U * iters), 1), 8192);
  // (round 3: a floor of 1024-2048 blocks for the small 20^2 / 40^2 layers made the step slower,
  // profiles/r03s_bn_minblocks_ab.txt: the extra blocks wait for CU slots the side stream holds)
  return (npix + blocks - 1) / blocks;
}

// pixels per BN-backward reduce block.  Partial-sum rows = reduce blocks, at most 256 with the
// pipelined reduce loop (one block per CU; cap 128 / 256 / 384 / 512: 18.64 / 18.28 / 18.52 /
// 18.74 ms per YOLOv8-s step, interleaved, profiles/r03ze_bn_reduce_pipe_cap_ab.txt).  With the
// serial loop 512 was best (round 2: 1024 19.82 ms, 512 19.50, 256 19.53, 2048 20.33).  The fused
// reduce + finalize (one last block sums the whole table) also keeps rows <= 32768 / c (table
// <= 256 KB); the two-kernel path does not: that cap left 64-128 reduce blocks on 256 CUs for
// the 256/512-channel layers (interleaved A/B: YOLOv8-s 19.51 -> 19.26 ms, -l 61.7 -> 60.9 ms).
static long bwd_pix_per_block(long npix, int c, bool fused) {
  constexpr long cap = 256, cprod = 32768;
  const long ccap = fused ? std::max(32l, cprod / std::max(c, 1)) : cap;
  const long rows = std::max(1l, std::min(std::min(cap, ccap), (npix + 63) / 64));
  return (npix + rows - 1) / rows;
}

// The per-pixel passes over yms_bn_pass_job: PPB is the pass's pixels-per-block formula, the one place
// the block count and the per-block pixel ranges of a job, solo or grouped, come from.
template <long (*PPB)(const yms_bn_pass_job&)>
struct PixelPass {
  using Job = yms_bn_pass_job;
  using Dev = PassJob;
  static bool groupable(const Job&) { return true; }
  static unsigned blocks(const Job& j) { return pix_blocks(j.npix, PPB(j)); }
  static Dev dev(const Job& j) { return pass_job(j, PPB(j)); }
};

// two U-pixel iterations per thread: the forward affine pass (no side-stream work beside it) took
// 1.73 / 1.74 ms per YOLOv8-s step against 1.80 / 1.80 at four, 3.66-3.68 vs 3.70-3.73 ms on
// YOLO-MS-S (interleaved, profiles/r03y_affine_iters_ab.txt)
// software-pipelined loop: affine 1.72 -> 1.70 ms per YOLOv8-s step, 3.68 -> 3.57 ms on YOLO-MS-S,
// steps 18.20 -> 18.13 ms and 37.24 -> 37.12 ms over the serial loop (interleaved pairs; pipelined
// at 4 / 8 iterations slower, profiles/r03zg_affine_pipe_ab.txt)
static long affine_ppb(const yms_bn_pass_job& j) { return elem_ppb(j.npix, j.c, 2); }

struct AffinePass : PixelPass<affine_ppb> {  // y = act(z*scale + shift) (+ res)
  static yms_status check(const Job& j) {
    if (j.npix <= 0 || !j.z || !j.out || !vok(j.z_ld, j.z_off, j.c) || !vok(j.out_ld, j.out_off, j.c))
      return YMS_ERR_INVALID;
    if (j.res && !vok(j.res_ld, j.res_off, j.c)) return YMS_ERR_INVALID;
    return j.c > 2048 ? YMS_ERR_UNSUPPORTED : YMS_OK;
  }
  static yms_status launch_solo(int dtype, const Job& j, hipStream_t st) {
    YMS_DT_DISPATCH(dtype, T, hipLaunchKernelGGL((affine_act_kernel<T, true>), dim3(blocks(j)), dim3(256), 0, st,
                                                 j.npix, j.c, (const T*)j.z, j.z_ld, j.z_off, j.scale, j.shift, j.act,
                                                 (const T*)j.res, j.res_ld, j.res_off, (T*)j.out, j.out_ld, j.out_off,
                                                 affine_ppb(j)));
    return launch_status();
  }
  static yms_status launch_group(int dtype, const BnGroup<Dev>& g, unsigned nb, hipStream_t st) {
    YMS_DT_DISPATCH(dtype, T, hipLaunchKernelGGL((affine_act_group_kernel<T, true>), dim3(nb), dim3(256), 0, st, g));
    return YMS_OK;
  }
};

// gy (and z) -> partial rows: the validation the reduce, the fused reduce + finalize and the bias
// reduce share (with_z: the BN + act reduce; fused: the in-launch finalize's arrival counter)
static yms_status reduce_check(const yms_bn_pass_job& j, bool with_z, bool fused) {
  if (j.npix <= 0 || !j.gy || !j.ws || (fused && !j.counter) || !vok(j.gy_ld, j.gy_off, j.c)) return YMS_ERR_INVALID;
  if (with_z && (!vok(j.z_ld, j.z_off, j.c) || !j.scale || !j.shift || !j.mean_invstd)) return YMS_ERR_INVALID;
  return j.c > 2048 ? YMS_ERR_UNSUPPORTED : YMS_OK;
}

static long reduce_ppb(const yms_bn_pass_job& j) { return bwd_pix_per_block(j.npix, j.c, false); }

struct ReducePass : PixelPass<reduce_ppb> {  // backward: partial sums of da and da*xhat -> ws
  static yms_status check(const Job& j) { return reduce_check(j, j.z != nullptr, false); }
  static bool groupable(const Job& j) { return j.z != nullptr; }   // the plain column sum: solo
  static yms_status launch_solo(int dtype, const Job& j, hipStream_t st) {
    // software-pipelined loop (c % 8 == 0).  At 512 rows it was step-neutral over the serial loop
    // (the reduce -10%, the apply after it +5%, profiles/r03zb_bn_reduce_pipe_ab.txt); with the
    // latency hidden inside each block, half the blocks (256 rows, bwd_pix_per_block) win: YOLOv8-s
    // 18.63 -> 18.32 ms/step, YOLO-MS-S 37.42 -> 37.28 ms (means of four interleaved runs each,
    // profiles/r03zd_*, r03ze_*); serial at 256 rows is slower.
#define YMS_RED(HZ)                                                                                                \
  YMS_DT_DISPATCH(dtype, T, hipLaunchKernelGGL((bn_bwd_reduce_kernel<T, HZ, false, true>), dim3(blocks(j)), dim3(256), \
                                               0, st, j.npix, j.c, HZ ? (const T*)j.z : (const T*)nullptr,         \
                                               HZ ? j.z_ld : 0, HZ ? j.z_off : 0, (const T*)j.gy, j.gy_ld, j.gy_off, \
                                               j.scale, j.shift, j.mean_invstd, j.act, j.ws, reduce_ppb(j)))
    if (j.z) YMS_RED(true);
    else YMS_RED(false);
#undef YMS_RED
    return launch_status();
  }
  static yms_status launch_group(int dtype, const BnGroup<Dev>& g, unsigned nb, hipStream_t st) {
    YMS_DT_DISPATCH(dtype, T, hipLaunchKernelGGL(bn_bwd_reduce_group_kernel<T>, dim3(nb), dim3(256), 0, st, g));
    return YMS_OK;
  }
};

struct BwdFinalizePass {                     // backward: partial rows -> dgamma, dbeta, the apply's coefficients
  using Job = yms_bn_bwd_finalize_job;
  using Dev = BwdFinJob;
  static yms_status check(const Job& j) {
    return j.c <= 0 || !j.ws || j.rows <= 0 || j.count <= 0 ? YMS_ERR_INVALID : YMS_OK;
  }
  static bool groupable(const Job&) { return true; }
  static unsigned blocks(const Job& j) { return (unsigned)cdiv(j.c, 32); }
  static Dev dev(const Job& j) { return BwdFinJob{j.c, j.rows, j.ws, j.count, j.dgamma, j.dbeta, j.coef}; }
  static yms_status launch_solo(int, const Job& j, hipStream_t st) {
    // (tried and dropped: float4 channel quads x 32 row lanes with every load of a lane in flight --
    // 19.42 -> 19.65 ms; a latency-shaped 8-channel x 32-lane variant with 4x the blocks -- +0.15-0.3
    // ms, profiles/r03q_bn_finalize_ab.txt: inside the step the finalize waits for CU slots, not loads)
    hipLaunchKernelGGL(bn_bwd_finalize_kernel<8>, dim3(blocks(j)), dim3(256), 0, st, j.c, j.ws, j.rows, j.count,
                       j.dgamma, j.dbeta, j.coef);
    return launch_status();
  }
  static yms_status launch_group(int, const BnGroup<Dev>& g, unsigned nb, hipStream_t st) {
    hipLaunchKernelGGL(bn_bwd_finalize_group_kernel<8>, dim3(nb), dim3(256), 0, st, g);
    return YMS_OK;
  }
};

// software-pipelined loop at eight U-pixel iterations per thread (half the blocks of the serial
// loop's best, four): YOLO-MS-S 37.27 -> 37.11 ms/step, YOLOv8-s 18.53 -> 18.49 ms (means of
// two interleaved runs; 4 / 16 iterations pipelined are slower, profiles/r03zf_bn_apply_pipe_ab.txt)
static long apply_ppb(const yms_bn_pass_job& j) {
  return elem_ppb(j.npix, j.c, 8 * BN_U / BN_UA);    // the same pixels per block at any U
}

struct ApplyPass : PixelPass<apply_ppb> {    // backward: dz over z (+ the residual's gradient)
  static yms_status check(const Job& j) {
    if (j.npix <= 0 || !j.z || !j.gy || !j.out || !j.scale || !j.shift || !j.mean_invstd || !j.coef)
      return YMS_ERR_INVALID;
    if (!vok(j.z_ld, j.z_off, j.c) || !vok(j.gy_ld, j.gy_off, j.c) || !vok(j.out_ld, j.out_off, j.c))
      return YMS_ERR_INVALID;
    if (j.res && !vok(j.res_ld, j.res_off, j.c)) return YMS_ERR_INVALID;
    return j.c > 2048 ? YMS_ERR_UNSUPPORTED : YMS_OK;
  }
  static yms_status launch_solo(int dtype, const Job& j, hipStream_t st) {
    YMS_DT_DISPATCH(dtype, T, hipLaunchKernelGGL((bn_bwd_apply_kernel<T, true>), dim3(blocks(j)), dim3(256), 0, st,
                                                 j.npix, j.c, (const T*)j.z, j.z_ld, j.z_off, (const T*)j.gy, j.gy_ld,
                                                 j.gy_off, j.scale, j.shift, j.mean_invstd, j.coef, j.act, (T*)j.out,
                                                 j.out_ld, j.out_off, (T*)j.res, j.res_ld, j.res_off, j.res_acc,
                                                 apply_ppb(j)));
    return launch_status();
  }
  static yms_status launch_group(int dtype, const BnGroup<Dev>& g, unsigned nb, hipStream_t st) {
    YMS_DT_DISPATCH(dtype, T, hipLaunchKernelGGL((bn_bwd_apply_group_kernel<T, true>), dim3(nb), dim3(256), 0, st, g));
    return YMS_OK;
  }
};

// reduce + finalize in one launch (the last block to arrive sums the table): yms_bn_act_bwd_reduce_finalize,
// and the bias pass, which is its z-less form
static long fused_ppb(const yms_bn_pass_job& j) { return bwd_pix_per_block(j.npix, j.c, true); }

static yms_status launch_reduce_finalize(int dtype, const yms_bn_pass_job& j, bool with_z, const BwdFin& fin,
                                         hipStream_t st) {
  const long ppb = fused_ppb(j);
  const unsigned rows = pix_blocks(j.npix, ppb);
  if (with_z) {
    YMS_DT_DISPATCH(dtype, T, hipLaunchKernelGGL((bn_bwd_reduce_kernel<T, true, true>), dim3(rows), dim3(256), 0, st,
                                                 j.npix, j.c, (const T*)j.z, j.z_ld, j.z_off, (const T*)j.gy, j.gy_ld,
                                                 j.gy_off, j.scale, j.shift, j.mean_invstd, j.act, j.ws, ppb, fin));
  } else {
    YMS_DT_DISPATCH(dtype, T, hipLaunchKernelGGL((bn_bwd_reduce_kernel<T, false, true>), dim3(rows), dim3(256), 0, st,
                                                 j.npix, j.c, (const T*)nullptr, 0, 0, (const T*)j.gy, j.gy_ld,
                                                 j.gy_off, j.scale, j.shift, j.mean_invstd, j.act, j.ws, ppb, fin));
  }
  return launch_status();
}

struct BiasPass {                            // dbias = sum over pixels of gy: reads gy, ws, counter, dbias of the job
  using Job = yms_bn_pass_job;
  using Dev = BiasJob;
  static yms_status check(const Job& j) { return reduce_check(j, false, true); }
  static bool groupable(const Job&) { return true; }
  static unsigned blocks(const Job& j) { return pix_blocks(j.npix, fused_ppb(j)); }
  static BwdFin fin(const Job& j) { return BwdFin{j.counter, nullptr, j.dbias, nullptr, j.npix}; }
  static Dev dev(const Job& j) { return BiasJob{j.npix, fused_ppb(j), j.c, j.gy, j.gy_ld, j.gy_off, j.ws, fin(j)}; }
  static yms_status launch_solo(int dtype, const Job& j, hipStream_t st) {
    // (without z the kernel reads none of the job's z, scale, shift, mean_invstd, act: null / 0 in a bias job)
    return launch_reduce_finalize(dtype, j, false, fin(j), st);
  }
  static yms_status launch_group(int dtype, const BnGroup<Dev>& g, unsigned nb, hipStream_t st) {
    YMS_DT_DISPATCH(dtype, T, hipLaunchKernelGGL(bias_bwd_group_kernel<T>, dim3(nb), dim3(256), 0, st, g));
    return YMS_OK;
  }
};

extern "C" {

yms_status yms_bn_finalize_ld(int c, float* stats, int rows, int stats_ld, long count,
                              const float* gamma, const float* beta, float* rmean, float* rvar,
                              float momentum, float eps, float* mean_invstd, int mi_ld, float* scale,
                              float* shift, void* stream) {
  const yms_bn_finalize_job j{c, stats, rows, stats_ld, count, gamma, beta, rmean, rvar, momentum, eps,
                              mean_invstd, mi_ld, scale, shift};
  return run_pass<FinalizePass>(0, 1, &j, stream);
}

yms_status yms_bn_finalize(int c, float* stats, int rows, int stats_ld, long count,
                           const float* gamma, const float* beta, float* rmean, float* rvar,
                           float momentum, float eps, float* mean_invstd, float* scale,
                           float* shift, void* stream) {
  return yms_bn_finalize_ld(c, stats, rows, stats_ld, count, gamma, beta, rmean, rvar, momentum, eps,
                            mean_invstd, c, scale, shift, stream);
}

yms_status yms_affine_act(int dtype, long npix, int c, const void* z, int z_ld, int z_off,
                          const float* scale, const float* shift, int act,
                          const void* res, int res_ld, int res_off,
                          void* y, int y_ld, int y_off, void* stream) {
  const yms_bn_pass_job j{npix, c, z, z_ld, z_off, nullptr, 0, 0, scale, shift, nullptr, nullptr, act, y, y_ld, y_off,
                          (void*)res, res_ld, res_off};
  return run_pass<AffinePass>(dtype, 1, &j, stream);
}

// the number of partial rows the reduce WRITES = its launched block count ceil(npix / ppb).
// Once a cap applies this can be below the cap (npix = 44801, c = 64: ppb 176, 255 blocks), so the
// scratch size, the launch and the finalize all use this one function.
int yms_bn_bwd_rows(long npix, int c) {
  if (npix <= 0 || c <= 0) return 0;
  return (int)pix_blocks(npix, bwd_pix_per_block(npix, c, false));   // >= the fused path's rows: sizes both
}

yms_status yms_bn_act_bwd_reduce(int dtype, long npix, int c, const void* z, int z_ld, int z_off,
                                 const void* gy, int gy_ld, int gy_off, const float* scale,
                                 const float* shift, const float* mean_invstd, int act,
                                 float* ws, void* stream) {
  const yms_bn_pass_job j{npix, c, z, z_ld, z_off, gy, gy_ld, gy_off, scale, shift, mean_invstd, nullptr, act,
                          nullptr, 0, 0, nullptr, 0, 0, 0, ws};
  return run_pass<ReducePass>(dtype, 1, &j, stream);
}

yms_status yms_bn_act_bwd_finalize(int c, const float* ws, int rows, long count, float* dgamma,
                                   float* dbeta, float* coef, void* stream) {
  const yms_bn_bwd_finalize_job j{c, ws, rows, count, dgamma, dbeta, coef};
  return run_pass<BwdFinalizePass>(0, 1, &j, stream);
}

yms_status yms_bn_act_bwd_apply(int dtype, long npix, int c, const void* z, int z_ld, int z_off,
                                const void* gy, int gy_ld, int gy_off, const float* scale,
                                const float* shift, const float* mean_invstd, const float* coef,
                                int act, void* dz, int dz_ld, int dz_off,
                                void* gres, int gres_ld, int gres_off, int gres_acc, void* stream) {
  const yms_bn_pass_job j{npix, c, z, z_ld, z_off, gy, gy_ld, gy_off, scale, shift, mean_invstd, coef, act,
                          dz, dz_ld, dz_off, gres, gres_ld, gres_off, gres_acc};
  return run_pass<ApplyPass>(dtype, 1, &j, stream);
}

yms_status yms_bn_act_bwd_reduce_finalize(int dtype, long npix, int c, const void* z, int z_ld, int z_off,
                                          const void* gy, int gy_ld, int gy_off, const float* scale,
                                          const float* shift, const float* mean_invstd, int act, float* ws,
                                          unsigned* counter, float* dgamma, float* dbeta, float* coef,
                                          void* stream) {
  const yms_bn_pass_job j{npix, c, z, z_ld, z_off, gy, gy_ld, gy_off, scale, shift, mean_invstd, nullptr, act,
                          nullptr, 0, 0, nullptr, 0, 0, 0, ws, counter};
  if (yms_status e = reduce_check(j, z != nullptr, true)) return e;
  return launch_reduce_finalize(dtype, j, z != nullptr, BwdFin{counter, dgamma, dbeta, coef, npix}, (hipStream_t)stream);
}

yms_status yms_bias_bwd(int dtype, long npix, int c, const void* gy, int gy_ld, int gy_off,
                        float* ws, unsigned* counter, float* dbias, void* stream) {
  const yms_bn_pass_job j{npix, c, nullptr, 0, 0, gy, gy_ld, gy_off, nullptr, nullptr, nullptr, nullptr, YMS_ACT_NONE,
                          nullptr, 0, 0, nullptr, 0, 0, 0, ws, counter, dbias};
  return run_pass<BiasPass>(dtype, 1, &j, stream);
}

yms_status yms_bn_finalize_group(int njobs, const yms_bn_finalize_job* jobs, void* stream) {
  return run_pass<FinalizePass>(0, njobs, jobs, stream);
}
yms_status yms_affine_act_group(int dtype, int njobs, const yms_bn_pass_job* jobs, void* stream) {
  return run_pass<AffinePass>(dtype, njobs, jobs, stream);
}
yms_status yms_bn_act_bwd_reduce_group(int dtype, int njobs, const yms_bn_pass_job* jobs, void* stream) {
  return run_pass<ReducePass>(dtype, njobs, jobs, stream);
}
yms_status yms_bn_act_bwd_finalize_group(int njobs, const yms_bn_bwd_finalize_job* jobs, void* stream) {
  return run_pass<BwdFinalizePass>(0, njobs, jobs, stream);
}
yms_status yms_bn_act_bwd_apply_group(int dtype, int njobs, const yms_bn_pass_job* jobs, void* stream) {
  return run_pass<ApplyPass>(dtype, njobs, jobs, stream);
}
yms_status yms_bias_bwd_group(int dtype, int njobs, const yms_bn_pass_job* jobs, void* stream) {
  return run_pass<BiasPass>(dtype, njobs, jobs, stream);
}

// With sums the blocks are the two-kernel reduce's (one partial row each: yms_bn_bwd_rows rows, the
// bound of ws); without, the apply pass's (a plain streaming pass, no ws, no counter).
yms_status yms_bn_frozen_act_bwd(int dtype, long npix, int c, const void* z, int z_ld, int z_off,
                                 const void* gy, int gy_ld, int gy_off, const float* scale,
                                 const float* shift, const float* mean_invstd, int act, void* dz, int dz_ld,
                                 int dz_off, void* gres, int gres_ld, int gres_off, int gres_acc, float* ws,
                                 unsigned* counter, float* dgamma, float* dbeta, void* stream) {
  const yms_bn_pass_job j{npix, c, z, z_ld, z_off, gy, gy_ld, gy_off, scale, shift, mean_invstd, nullptr, act,
                          dz, dz_ld, dz_off, gres, gres_ld, gres_off, gres_acc, ws, counter, dbeta};
  const bool sums = dgamma || dbeta;
  if (npix <= 0 || !z || !gy || !dz || !scale || !shift) return YMS_ERR_INVALID;
  if (!vok(z_ld, z_off, c) || !vok(gy_ld, gy_off, c) || !vok(dz_ld, dz_off, c)) return YMS_ERR_INVALID;
  if (gres && !vok(gres_ld, gres_off, c)) return YMS_ERR_INVALID;
  if (sums && (!mean_invstd || !ws || !counter)) return YMS_ERR_INVALID;
  if (c > 2048) return YMS_ERR_UNSUPPORTED;
  const long ppb = sums ? reduce_ppb(j) : apply_ppb(j);
  const PassJob pj = pass_job(j, ppb);
  const BwdFin fin{counter, dgamma, dbeta, nullptr, npix};
  const dim3 grid(pix_blocks(npix, ppb));
  hipStream_t st = (hipStream_t)stream;
  if (sums) YMS_DT_DISPATCH(dtype, T, hipLaunchKernelGGL((bn_frozen_bwd_kernel<T, true>), grid, dim3(256), 0, st, pj, fin));
  else YMS_DT_DISPATCH(dtype, T, hipLaunchKernelGGL((bn_frozen_bwd_kernel<T, false>), grid, dim3(256), 0, st, pj, fin));
  return launch_status();
}

// yms_bn_fold plus the [2][mi_ld] (running_mean, invstd) table; the batched form runs njobs layers'
// folds in one launch from a DEVICE table of yms_bn_fold_job whose outputs are byte offsets from base.
yms_status yms_bn_fold_mi(int c, const float* gamma, const float* beta, const float* rmean, const float* rvar,
                          float eps, float* scale, float* shift, float* mean_invstd, int mi_ld, void* stream) {
  if (c <= 0 || !gamma || !beta || !rmean || !rvar || !scale || !shift || !mean_invstd || mi_ld < c)
    return YMS_ERR_INVALID;
  const FoldJob j{gamma, beta, rmean, rvar, eps, c, mi_ld, (long)(intptr_t)scale, (long)(intptr_t)shift,
                  (long)(intptr_t)mean_invstd};
  hipLaunchKernelGGL(bn_fold_mi_kernel, dim3(cdiv(c, 256)), dim3(256), 0, (hipStream_t)stream, nullptr, j, nullptr);
  return launch_status();
}

yms_status yms_bn_fold_mi_batched(int njobs, const yms_bn_fold_job* jobs_dev, int max_c, void* base, void* stream) {
  static_assert(sizeof(yms_bn_fold_job) == sizeof(FoldJob), "yms_bn_fold_job is FoldJob");
  if (njobs < 0 || max_c <= 0 || (njobs > 0 && (!jobs_dev || !base))) return YMS_ERR_INVALID;
  if (njobs == 0) return YMS_OK;
  hipLaunchKernelGGL(bn_fold_mi_kernel, dim3(cdiv(max_c, 256), njobs), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const FoldJob*>(jobs_dev), FoldJob{}, (char*)base);
  return launch_status();
}

size_t yms_sppf_ws_bytes(int n, int h, int w, int c) {
  return (size_t)n * h * w * ((c + 7) / 8) * 8;
}

// The one-launch chain takes 16-bit planes whose backward fits SPPF_LDS_MAX (h * w <= 585); every
// other shape runs the three-launch kernels.
int yms_sppf_fused_fits(int dtype, int h, int w, int c) {
  if (dtype != YMS_BF16 && dtype != YMS_F16) return 0;
  if (h <= 0 || w <= 0 || c <= 0 || c % 8 != 0) return 0;
  const long p = (long)h * w;
  return p * SPPF_BWD_BPP <= SPPF_LDS_MAX && p <= 256 * SPPF_NP;
}
static int& sppf_route() {
  static int r = 1;
  return r;
}
int yms_sppf_route_set(int v) {
  const int prev = sppf_route();
  if (v >= 0) sppf_route() = v ? 1 : 0;
  return prev;
}

yms_status yms_sppf_pool_fwd(int dtype, int n, int h, int w, int c, void* buf, int ld, int off,
                             void* stream) {
  if (n <= 0 || h <= 0 || w <= 0 || !buf || !vok(ld, off, 4 * c) || c % 8 != 0) return YMS_ERR_INVALID;
  const long items = (long)n * h * w * ((c + 7) / 8);
  if (items >= (1l << 31)) return YMS_ERR_UNSUPPORTED;
  if (sppf_route() && yms_sppf_fused_fits(dtype, h, w, c)) {
    const int nlog = n * (c / 8);
    const dim3 grid((unsigned)rup(nlog, 8));
    const size_t lds = (size_t)h * w * 32;
    if (dtype == YMS_BF16)
      hipLaunchKernelGGL(sppf_chain_fwd_kernel<bf16>, grid, dim3(256), lds, (hipStream_t)stream, nlog, h, w, c,
                         (bf16*)buf, ld, off);
    else
      hipLaunchKernelGGL(sppf_chain_fwd_kernel<f16>, grid, dim3(256), lds, (hipStream_t)stream, nlog, h, w, c,
                         (f16*)buf, ld, off);
    return launch_status();
  }
  for (int k = 1; k <= 3; ++k)
    YMS_DT_DISPATCH(dtype, T, hipLaunchKernelGGL(pool5_fwd_kernel<T>, dim3(grid_for(items)), dim3(256), 0,
                                                 (hipStream_t)stream, n, h, w, c, (T*)buf, ld,
                                                 off + (k - 1) * c, off + k * c));
  return launch_status();
}

yms_status yms_sppf_pool_bwd(int dtype, int n, int h, int w, int c, const void* buf, int ld,
                             int off, void* gbuf, int gld, int goff, void* ws, void* stream) {
  if (n <= 0 || !buf || !gbuf || !ws || !vok(ld, off, 4 * c) || !vok(gld, goff, 4 * c) || c % 8 != 0)
    return YMS_ERR_INVALID;
  if (ld != gld) return YMS_ERR_UNSUPPORTED;
  const long items = (long)n * h * w * ((c + 7) / 8);
  if (items >= (1l << 31)) return YMS_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  // One launch for the three pools (sppf_chain_bwd_kernel) where the plane fits: 22 KB of LDS per
  // block at 20x20, so its blocks sit beside the side stream's weight gradients (the round-3 attempt,
  // one 64-KB-LDS launch per pool, lost 0.1 ms in the step waiting for that LDS,
  // profiles/r03v_sppf_fused_ab.txt).  In the step the chain's kernels take 424 -> 162 us and the
  // step 16.90 -> 16.64 ms (profiles/sppf_chain_stats_*.txt, sppf_chain_ab.txt).  The fused backward
  // is VALU-bound (94 % of the SIMDs' issue cycles, profiles/sppf_chain_micro.txt): the 25-tap
  // gather's compare / select / add per channel is what is left, not memory.
  if (sppf_route() && yms_sppf_fused_fits(dtype, h, w, c)) {
    const int nlog = n * (c / 8);
    const dim3 grid((unsigned)rup(nlog, 8));
    const size_t lds = (size_t)h * w * SPPF_BWD_BPP;
    if (dtype == YMS_BF16)
      hipLaunchKernelGGL(sppf_chain_bwd_kernel<bf16>, grid, dim3(256), lds, st, nlog, h, w, c, (const bf16*)buf, ld,
                         off, (bf16*)gbuf, gld, goff);
    else
      hipLaunchKernelGGL(sppf_chain_bwd_kernel<f16>, grid, dim3(256), lds, st, nlog, h, w, c, (const f16*)buf, ld,
                         off, (f16*)gbuf, gld, goff);
    return launch_status();
  }
  for (int k = 3; k >= 1; --k) {
    // pool k reads slot k-1 (value buf) and produced slot k; push grad of slot k into slot k-1
    YMS_DT_DISPATCH(dtype, T, {
      hipLaunchKernelGGL(pool5_argmax_kernel<T>, dim3(grid_for(items)), dim3(256), 0, st, n, h, w, c,
                         (const T*)buf, ld, off + (k - 1) * c, (uint8_t*)ws);
      hipLaunchKernelGGL(pool5_gather_kernel<T>, dim3(grid_for(items)), dim3(256), 0, st, n, h, w, c,
                         (const uint8_t*)ws, (T*)gbuf, gld, goff + (k - 1) * c, goff + k * c);
    });
  }
  return launch_status();
}

yms_status yms_upsample2x_fwd(int dtype, int n, int h, int w, int c, const void* x, int x_ld,
                              int x_off, void* y, int y_ld, int y_off, void* stream) {
  if (n <= 0 || !x || !y || !vok(x_ld, x_off, c) || !vok(y_ld, y_off, c)) return YMS_ERR_INVALID;
  const long items = (long)n * 4 * h * w * ((c + 7) / 8);
  YMS_DT_DISPATCH(dtype, T, hipLaunchKernelGGL(upsample_fwd_kernel<T>, dim3(grid_for(items)), dim3(256), 0,
                                               (hipStream_t)stream, n, h, w, c, (const T*)x, x_ld, x_off,
                                               (T*)y, y_ld, y_off));
  return launch_status();
}

yms_status yms_upsample2x_bwd(int dtype, int n, int h, int w, int c, const void* gy, int gy_ld,
                              int gy_off, void* gx, int gx_ld, int gx_off, int accumulate,
                              void* stream) {
  if (n <= 0 || !gy || !gx || !vok(gy_ld, gy_off, c) || !vok(gx_ld, gx_off, c)) return YMS_ERR_INVALID;
  const long items = (long)n * h * w * ((c + 7) / 8);
  YMS_DT_DISPATCH(dtype, T, hipLaunchKernelGGL(upsample_bwd_kernel<T>, dim3(grid_for(items)), dim3(256), 0,
                                               (hipStream_t)stream, n, h, w, c, (const T*)gy, gy_ld, gy_off,
                                               (T*)gx, gx_ld, gx_off, accumulate));
  return launch_status();
}

yms_status yms_pack_input(int dtype, int n, int c, int h, int w, const float* x, void* y, int ld,
                          void* stream) {
  if (n <= 0 || c <= 0 || !x || !y || ld % 8 != 0 || ld < c) return YMS_ERR_INVALID;
  const long npix = (long)n * h * w;
  YMS_DT_DISPATCH(dtype, T, hipLaunchKernelGGL(pack_input_kernel<T>, dim3(grid_for(npix)), dim3(256), 0,
                                               (hipStream_t)stream, n, c, h, w, x, (T*)y, ld));
  return launch_status();
}

#define YMS_DT2(d1, d2, T1, T2, ...)                                          \
  YMS_DT_DISPATCH(d1, T1, { YMS_DT_DISPATCH(d2, T2, __VA_ARGS__); })

yms_status yms_nhwc_to_nchw(int dtype, int dtype_nchw, int n, int h, int w, int c, const void* x,
                            int ld, int off, void* y, void* stream) {
  if (n <= 0 || h <= 0 || w <= 0 || !x || !y || !vok(ld, off, c)) return YMS_ERR_INVALID;
  const long hw = (long)h * w;
  dim3 grid((unsigned)cdiv(hw, 64), (unsigned)cdiv(c, 64), (unsigned)n);
  YMS_DT2(dtype, dtype_nchw, TI, TO, hipLaunchKernelGGL((nhwc_to_nchw_kernel<TI, TO>), grid, dim3(256), 0,
                                                        (hipStream_t)stream, n, hw, c, (const TI*)x, ld, off,
                                                        (TO*)y));
  return launch_status();
}

yms_status yms_nchw_to_nhwc(int dtype_nchw, int dtype, int n, int h, int w, int c, const void* x,
                            void* y, int ld, int off, int accumulate, void* stream) {
  if (n <= 0 || h <= 0 || w <= 0 || !x || !y || !vok(ld, off, c)) return YMS_ERR_INVALID;
  const long hw = (long)h * w;
  dim3 grid((unsigned)cdiv(hw, 64), (unsigned)cdiv(c, 64), (unsigned)n);
  YMS_DT2(dtype_nchw, dtype, TI, TO, hipLaunchKernelGGL((nchw_to_nhwc_kernel<TI, TO>), grid, dim3(256), 0,
                                                        (hipStream_t)stream, n, hw, c, (const TI*)x, (TO*)y,
                                                        ld, off, accumulate));
  return launch_status();
}

yms_status yms_cast(int dtype_in, int dtype_out, long count, const void* x, void* y, void* stream) {
  if (count <= 0 || !x || !y) return YMS_ERR_INVALID;
  YMS_DT2(dtype_in, dtype_out, TI, TO, hipLaunchKernelGGL((cast_kernel<TI, TO>), dim3(grid_for(count)),
                                                          dim3(256), 0, (hipStream_t)stream, count,
                                                          (const TI*)x, (TO*)y));
  return launch_status();
}

}  // extern "C"

extern "C" yms_status yms_zero(void* p, size_t bytes, void* stream) {
  if (!p) return YMS_ERR_INVALID;
  if (bytes == 0) return YMS_OK;
  return hipMemsetAsync(p, 0, bytes, (hipStream_t)stream) == hipSuccess ? YMS_OK : YMS_ERR_LAUNCH;
}

extern "C" yms_status yms_copy(void* dst, const void* src, size_t bytes, void* stream) {
  if (!dst || !src) return YMS_ERR_INVALID;
  if (bytes == 0) return YMS_OK;
  return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream) == hipSuccess
             ? YMS_OK : YMS_ERR_LAUNCH;
}
