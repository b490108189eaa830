// COCOeval.accumulate on the device (yms_map_accumulate_coco_dev): the precision[T][101][K][4][3] and
// recall[T][K][4][3] tables of yms_map_accumulate_coco (csrc/map_eval.hip, the definition), cell for
// cell, from the epoch buffers that yms_map_match_coco_fixed fills -- no host read, no allocation, a
// fixed launch sequence per (n_rows, K).
//
//   1. fill: both tables = -1.
//   2. key:  key[row] = class << 32 | ~flip(score), flip = the order-preserving bit flip of an fp32
//            (-0 counted as +0), so ascending keys are (class ascending, score descending); rows that
//            take no part (dead, rank >= 100, label outside [0, K)) get the sentinel class K and sort
//            last.  value[row] = row.
//   3. sort: stable LSD radix sort of (key, row), 8 bits a pass over the 32 + bit_length(K) key bits
//            (three launches a pass: per-wave digit histogram, one-block exclusive scan of the
//            digit-major counts, stable scatter).  Rows start in ascending order and every pass is
//            stable, so equal (class, score) stay in row = (image, index) order: the host's order.
//   4. accumulate: one wave per (class, maxDet); lane = area * 16 + threshold, as in the matcher.  The
//            class' segment of the sorted rows (two binary searches) is walked twice in chunks of 64
//            rows whose masks the wave gathers into LDS: forward to count each lane's tp and fp
//            (integers), backward undoing them row by row, which gives every row's running counts
//            without storing any.  A row outside the maxDet, or ignored, changes no count.
//
// Why the backward walk needs a division only at true positives: the host samples the reverse running
// maximum of pr at lower_bound(rc, r / 100).  rc = tp / npig depends on tp alone, so the sample for r
// is the maximum of pr over the rows whose tp >= vmin(r), the smallest count with vmin / npig >= r * 0.01
// (found with the same fp64 division and comparison the host makes).  Among rows of equal tp the
// first has the fewest false positives and x / (fp + x + eps) does not grow with fp under correctly
// rounded fp64, so the maximum over a set of rows is the maximum over its true-positive rows: the same
// set of doubles, and a maximum has no rounding.  tp / npig and tp / (fp + tp + eps) are single fp64
// divisions of exactly represented integers: bit-identical to the host.
#include <algorithm>
#include <climits>

#include "yms_common.hpp"

namespace yms {

constexpr int ACC_MAX_THR = 16;
constexpr int ACC_N_AREA = 4;
constexpr int ACC_N_MD = 3;
constexpr int ACC_N_REC = 101;
constexpr int ACC_MAXDET = 100;
constexpr int ACC_MAX_CLASSES = 4096;
constexpr int ACC_CHUNK = 64;         // sorted rows staged in LDS per step of the two walks
constexpr int SORT_WAVES = 4;
constexpr int SORT_TILE = 2048;       // rows per wave and pass

__global__ __launch_bounds__(256) void map_acc_fill_kernel(double* precision, long n_prec, double* recall,
                                                           long n_rec) {
  const long step = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n_prec + n_rec; i += step) {
    if (i < n_prec) precision[i] = -1.0;
    else recall[i - n_prec] = -1.0;
  }
}

__global__ __launch_bounds__(256) void map_acc_key_kernel(int n, const float* score, const int* label,
                                                          const int* rank, int K, uint64_t* keys, unsigned* vals) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int lab = label[i], rk = rank[i];
  const bool on = rk >= 0 && rk < ACC_MAXDET && lab >= 0 && lab < K;
  unsigned b = __float_as_uint(score[i]);
  if (b == 0x80000000u) b = 0u;                                  // -0 == +0 in the host's comparison
  const unsigned asc = b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
  keys[i] = ((uint64_t)(unsigned)(on ? lab : K) << 32) | (uint64_t)(~asc);
  vals[i] = (unsigned)i;
}

// hist[digit * units + unit] = the number of the unit's rows with that digit (unit = one wave's tile)
__global__ __launch_bounds__(64 * SORT_WAVES) void map_sort_hist_kernel(int n, const uint64_t* keys, int shift,
                                                                        unsigned* hist, int units) {
  __shared__ unsigned cnt[SORT_WAVES][256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int u = blockIdx.x * SORT_WAVES + wave;
  for (int d = lane; d < 256; d += 64) cnt[wave][d] = 0u;
  __syncthreads();
  const long base = (long)u * SORT_TILE;
  for (int k = lane; k < SORT_TILE; k += 64) {
    const long i = base + k;
    if (i < n) atomicAdd(&cnt[wave][(unsigned)(keys[i] >> shift) & 255u], 1u);
  }
  __syncthreads();
  if (u < units)
    for (int d = lane; d < 256; d += 64) hist[(long)d * units + u] = cnt[wave][d];
}

// in-place exclusive scan of hist[0 .. total) by one workgroup, 1024 entries a step
__global__ __launch_bounds__(1024) void map_sort_scan_kernel(unsigned* hist, int total) {
  __shared__ unsigned wsum[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned carry = 0u;
  for (int base = 0; base < total; base += 1024) {
    const int i = base + tid;
    const unsigned x = i < total ? hist[i] : 0u;
    unsigned s = x;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
      const unsigned o = __shfl_up(s, m);
      if (lane >= m) s += o;
    }
    if (lane == 63) wsum[wave] = s;
    __syncthreads();
    unsigned before = 0u, all = 0u;
#pragma unroll
    for (int w = 0; w < 16; ++w) {
      const unsigned v = wsum[w];
      before += w < wave ? v : 0u;
      all += v;
    }
    if (i < total) hist[i] = carry + before + s - x;
    carry += all;
    __syncthreads();
  }
}

// Stable scatter: a wave takes its tile 64 rows at a time in order; a row's place is the unit's running
// offset for its digit plus the number of lower lanes with the same digit (eight ballots).
__global__ __launch_bounds__(64 * SORT_WAVES) void map_sort_scatter_kernel(int n, const uint64_t* kin,
                                                                           const unsigned* vin, uint64_t* kout,
                                                                           unsigned* vout, int shift,
                                                                           const unsigned* offs, int units) {
  __shared__ unsigned off[SORT_WAVES][256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int u = blockIdx.x * SORT_WAVES + wave;
  for (int d = lane; d < 256; d += 64) off[wave][d] = u < units ? offs[(long)d * units + u] : 0u;
  __syncthreads();
  const long base = (long)u * SORT_TILE;
  for (int k = 0; k < SORT_TILE; k += 64) {          // the same trip count in every wave: the barriers are uniform
    const long i = base + k + lane;
    const bool valid = i < n;
    uint64_t key = 0;
    unsigned val = 0u;
    if (valid) {
      key = kin[i];
      val = vin[i];
    }
    const unsigned dg = (unsigned)(key >> shift) & 255u;
    unsigned long long same = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (dg >> b) & 1u;
      const unsigned long long bb = __ballot(valid && bit);
      same &= bit ? bb : ~bb;
    }
    const int before = __popcll(same & ((1ull << lane) - 1ull));
    const unsigned pos = valid ? off[wave][dg] + (unsigned)before : 0u;
    __syncthreads();
    if (valid && before == __popcll(same) - 1) off[wave][dg] = pos + 1u;
    __syncthreads();
    if (valid && pos < (unsigned)n) {                 // pos < n by construction; never store past the buffers
      kout[pos] = key;
      vout[pos] = val;
    }
  }
}

// One wave per (class, maxDet), lane = area * 16 + threshold.  See the head of the file.
__global__ __launch_bounds__(64) void map_acc_kernel(int n, long cap, const uint64_t* keys, const unsigned* rows,
                                                     const int* rank, const uint16_t* matched,
                                                     const uint16_t* ignored, int T, int K, const int* npig,
                                                     double* precision, double* recall) {
#pragma clang fp contract(off)
  __shared__ int vmin[ACC_N_AREA][ACC_N_REC + 3];
  __shared__ unsigned stage[ACC_N_AREA][ACC_CHUNK];
  const int lane = threadIdx.x, t = lane & 15, a = lane >> 4;
  const int c = blockIdx.x / ACC_N_MD, mi = blockIdx.x % ACC_N_MD;
  const int md = mi == 0 ? 1 : (mi == 1 ? 10 : ACC_MAXDET);
  bool any = false;
  for (int x = 0; x < ACC_N_AREA; ++x) any = any || npig[c * ACC_N_AREA + x] > 0;
  if (!any) return;                                   // block-uniform: the cells keep their -1
  const int np = npig[c * ACC_N_AREA + a];
  const bool live = t < T && np > 0;
  const double dn = (double)np;
  // vmin[area][r]: the smallest true-positive count whose recall reaches r * 0.01
  for (int idx = lane; idx < ACC_N_AREA * ACC_N_REC; idx += 64) {
    const int a2 = idx / ACC_N_REC, r = idx % ACC_N_REC;
    const int n2 = npig[c * ACC_N_AREA + a2];
    long g = 0;
    if (n2 > 0) {
      const double thr = (double)r * 0.01, d2 = (double)n2;     // np.linspace(0, 1, 101) = arange(101) * 0.01
      g = (long)ceil(thr * d2);
      g = g < 0 ? 0 : (g > n2 ? (long)n2 : g);
      while (g > 0 && (double)(g - 1) / d2 >= thr) --g;
      while ((double)g / d2 < thr) ++g;
    }
    vmin[a2][r] = (int)g;
  }
  __syncthreads();
  // the class' segment of the sorted rows
  int seg[2];
  for (int k = 0; k < 2; ++k) {
    const uint64_t target = (uint64_t)(unsigned)(c + k) << 32;
    int lo = 0, hi = n;
    while (lo < hi) {
      const int mid = (int)(((long)lo + hi) >> 1);
      if (keys[mid] < target) lo = mid + 1;
      else hi = mid;
    }
    seg[k] = lo;
  }
  const int s = seg[0], e = seg[1];

  // gather the masks of the chunk's rows: matched | ignored << 16 per area; a row beyond the maxDet
  // (or past the segment) counts as ignored at every threshold
  auto gather = [&](int base) {
    unsigned x[ACC_N_AREA];
#pragma unroll
    for (int a2 = 0; a2 < ACC_N_AREA; ++a2) x[a2] = 0xffff0000u;
    const int i = base + lane;
    if (i < e) {
      const unsigned row = rows[i];
      if (row < (unsigned)n) {
        const int rk = rank[row];
        if (rk >= 0 && rk < md) {
#pragma unroll
          for (int a2 = 0; a2 < ACC_N_AREA; ++a2)
            x[a2] = (unsigned)matched[a2 * cap + row] | ((unsigned)ignored[a2 * cap + row] << 16);
        }
      }
    }
#pragma unroll
    for (int a2 = 0; a2 < ACC_N_AREA; ++a2) stage[a2][lane] = x[a2];
    __syncthreads();
  };

  int tpc = 0, fpc = 0;
  for (int base = s; base < e; base += ACC_CHUNK) {
    gather(base);
    const int cnt = min(ACC_CHUNK, e - base);
    for (int j = 0; j < cnt; ++j) {
      const unsigned x = stage[a][j];
      const unsigned m = (x >> t) & 1u, ig = (x >> (16 + t)) & 1u;
      tpc += (int)(m & (ig ^ 1u));
      fpc += (int)((m ^ 1u) & (ig ^ 1u));
    }
    __syncthreads();
  }

  const double eps = 0x1p-52;                          // np.spacing(1)
  const long rstride = (long)K * ACC_N_AREA * ACC_N_MD;
  double* pcell = precision + ((((long)t * ACC_N_REC) * K + c) * ACC_N_AREA + a) * ACC_N_MD + mi;
  int rptr = ACC_N_REC - 1;
  if (live) {
    recall[(((long)t * K + c) * ACC_N_AREA + a) * ACC_N_MD + mi] = (double)tpc / dn;
    while (rptr >= 1 && vmin[a][rptr] > tpc) {         // recall levels never reached
      pcell[rptr * rstride] = 0.0;
      --rptr;
    }
  }
  double env = 0.0;
  for (int ch = (e - s + ACC_CHUNK - 1) / ACC_CHUNK - 1; ch >= 0; --ch) {
    const int base = s + ch * ACC_CHUNK;
    gather(base);
    const int cnt = min(ACC_CHUNK, e - base);
    for (int j = cnt - 1; j >= 0; --j) {
      const unsigned x = stage[a][j];
      const unsigned m = (x >> t) & 1u, ig = (x >> (16 + t)) & 1u;
      if (ig) continue;
      if (m) {
        if (live) {
          const double p = (double)tpc / (((double)fpc + (double)tpc) + eps);
          env = p > env ? p : env;
          while (rptr >= 1 && vmin[a][rptr] == tpc) {  // the rows from here on are the first to reach level rptr
            pcell[rptr * rstride] = env;
            --rptr;
          }
        }
        --tpc;
      } else {
        --fpc;
      }
    }
    __syncthreads();
  }
  if (live) pcell[0] = env;                            // r = 0: every row
}

static int key_passes(int n_classes) {
  int bits = 32;
  for (unsigned k = (unsigned)n_classes; k; k >>= 1) ++bits;      // classes 0 .. K, the sentinel included
  return (bits + 7) / 8;
}

struct AccWs {
  size_t keys[2], vals[2], hist, total;
  int units;
};

static AccWs acc_ws(long n_rows) {
  AccWs w;
  const long n = n_rows > 0 ? n_rows : 0;
  w.units = cdiv(n, SORT_TILE);
  size_t o = 0;
  for (int k = 0; k < 2; ++k) { w.keys[k] = o; o += (size_t)rup(n * 8, 256); }
  for (int k = 0; k < 2; ++k) { w.vals[k] = o; o += (size_t)rup(n * 4, 256); }
  w.hist = o;
  o += (size_t)rup((long)w.units * 256 * 4, 256);
  w.total = o + 256;
  return w;
}

}  // namespace yms

using namespace yms;

extern "C" {

size_t yms_map_accumulate_coco_dev_ws_bytes(long n_rows, int n_thr, int n_classes) {
  (void)n_thr;
  (void)n_classes;
  return acc_ws(n_rows).total;
}

yms_status yms_map_accumulate_coco_dev(long n_rows, long cap, const float* score, const int* label, const int* rank,
                                       const uint16_t* matched, const uint16_t* ignored, int n_thr, int n_classes,
                                       const int* npig, double* precision, double* recall, void* ws, size_t ws_bytes,
                                       void* stream) {
  if (n_rows < 0 || n_rows > INT_MAX || cap < n_rows || n_thr < 1 || n_thr > ACC_MAX_THR || n_classes < 1 ||
      n_classes > ACC_MAX_CLASSES || !npig || !precision || !recall)
    return YMS_ERR_INVALID;
  if (n_rows > 0 && (!score || !label || !rank || !matched || !ignored || !ws)) return YMS_ERR_INVALID;
  const AccWs w = acc_ws(n_rows);
  if (n_rows > 0 && ws_bytes < w.total) return YMS_ERR_INVALID;
  hipStream_t st = (hipStream_t)stream;
  const int n = (int)n_rows, K = n_classes;
  const long n_prec = (long)n_thr * ACC_N_REC * K * ACC_N_AREA * ACC_N_MD, n_rec = (long)n_thr * K * ACC_N_AREA * ACC_N_MD;
  hipLaunchKernelGGL(map_acc_fill_kernel, dim3((unsigned)std::min<long>(cdiv(n_prec + n_rec, 256), 4096)), dim3(256), 0,
                     st, precision, n_prec, recall, n_rec);
  const uint64_t* keys = nullptr;
  const unsigned* rows = nullptr;
  if (n > 0) {
    char* base = (char*)ws;
    uint64_t* kb[2] = {(uint64_t*)(base + w.keys[0]), (uint64_t*)(base + w.keys[1])};
    unsigned* vb[2] = {(unsigned*)(base + w.vals[0]), (unsigned*)(base + w.vals[1])};
    unsigned* hist = (unsigned*)(base + w.hist);
    hipLaunchKernelGGL(map_acc_key_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, st, n, score, label, rank, K,
                       kb[0], vb[0]);
    const unsigned blocks = (unsigned)cdiv(w.units, SORT_WAVES);
    int cur = 0;
    for (int p = 0; p < key_passes(K); ++p, cur ^= 1) {
      hipLaunchKernelGGL(map_sort_hist_kernel, dim3(blocks), dim3(64 * SORT_WAVES), 0, st, n, kb[cur], 8 * p, hist,
                         w.units);
      hipLaunchKernelGGL(map_sort_scan_kernel, dim3(1), dim3(1024), 0, st, hist, w.units * 256);
      hipLaunchKernelGGL(map_sort_scatter_kernel, dim3(blocks), dim3(64 * SORT_WAVES), 0, st, n, kb[cur], vb[cur],
                         kb[cur ^ 1], vb[cur ^ 1], 8 * p, hist, w.units);
    }
    keys = kb[cur];
    rows = vb[cur];
  }
  hipLaunchKernelGGL(map_acc_kernel, dim3((unsigned)(K * ACC_N_MD)), dim3(64), 0, st, n, cap, keys, rows, rank, matched,
                     ignored, n_thr, K, npig, precision, recall);
  return launch_status();
}

}  // extern "C"
