// COCO-protocol detect for gfx950: the candidate stage in front of yms_nms_classwise and the
// finalize stage behind it (ultralytics non_max_suppression's protocol: multi-label candidates above
// conf, at most max_nms of them by score, class-wise or agnostic NMS, at most max_det detections by
// score, boxes mapped back through the letterbox and clipped).  Tie rules are this package's
// (parity with ultralytics UNPINNED: it leaves ties to its sort).
//
// Candidates.  A pair (anchor a, class c) with score > conf is a candidate; its key is the score's bit
// pattern (conf >= 0, so keys are positive floats and order as unsigned integers; 0 = no candidate)
// and its id is p = a * nc + c.  Per image the K best by (key descending, p ascending) survive and
// are stored in ascending p.  Everything is integer counting, so the output does not depend on
// which block runs first, and no block waits for another inside a launch:
//   memset      histograms and totals
//   count       per block: candidates -> blk_gt; per image: total, histogram of key bits 30..20
//   select 0    total <= K: no overflow, threshold 0.  Else the bin holding the K-th key
//   hist 1      overflowing images only: histogram of bits 19..9 under the chosen prefix
//   select 1
//   hist 2      bits 8..0
//   select 2    -> thr (the K-th key) and quota (how many candidates AT thr are admitted)
//   rank        overflowing images only: per block, keys > thr -> blk_gt, keys == thr -> blk_eq
//   write       a candidate's row is (keys > thr before it) + min(keys == thr before it, quota), "before"
//               in p order: block offsets from blk_gt / blk_eq, inside the block an ordered scan
// The launch count is fixed; blocks of images that need no select leave at once.  Each pass reads
// pred once: rows of 4 + nc floats, 16 lanes per anchor (nms_prep_kernel's walk), as float4 when
// nc % 4 == 0.
//
// Finalize.  One workgroup per image: the kept rows' unique 48-bit keys (score bits, then lower row
// first) go through a radix select when there are more than max_det, the survivors (<= 1024) are
// sorted in LDS, and the boxes are un-letterboxed with separately rounded fp32 operations.
//
// Box voting (yms_det_finalize_vote).  The same ranking, instantiated to leave each emitted
// detection's candidate row id in its box slot; a second launch then runs one wavefront per emitted
// detection over the image's live candidate rows, sums score * box and score in float64 over the rows
// of its NMS label that the NMS's own predicate (iou_gt, nms_pick.hpp) puts above the threshold, and
// overwrites the slot with the mean, un-letterboxed as above.  n * max_det wavefronts of at most K
// pair tests each, whatever the NMS kept.
#include "nms_pick.hpp"

#pragma clang fp contract(off)

namespace yms {

constexpr int DET_BINS = 2048;
constexpr int DET_MAXB = 256;       // blocks per image at most (the write kernel sums them with 256 threads)
constexpr int DET_MAX_K = 65536;
constexpr int DET_MAX_DET = 1024;

struct DetArgs {
  int A, nc, apb;                   // apb: anchors per block (a multiple of 16)
  const float* pred;
  float conf;
  const uint8_t* mask;              // NULL or [nc]: classes that may be candidates
};

struct DetWs {
  uint32_t* hist;                   // [3][n][DET_BINS]
  uint32_t* total;                  // [n] (right behind hist: one memset clears both)
  uint32_t* state;                  // [n][4]: overflow, prefix -> thr, remaining -> quota
  int* blk_gt;                      // [n][DET_MAXB]
  int* blk_eq;                      // [n][DET_MAXB]
};

static size_t det_r256(size_t x) { return (x + 255) & ~(size_t)255; }
static size_t det_ws_bytes(int n) {
  return det_r256(((size_t)3 * n * DET_BINS + n) * 4) + det_r256((size_t)n * 16) +
         2 * det_r256((size_t)n * DET_MAXB * 4);
}
static DetWs det_carve(void* ws, int n) {
  char* p = (char*)ws;
  DetWs w;
  w.hist = (uint32_t*)p;
  w.total = w.hist + (size_t)3 * n * DET_BINS;
  p += det_r256(((size_t)3 * n * DET_BINS + n) * 4);
  w.state = (uint32_t*)p;
  p += det_r256((size_t)n * 16);
  w.blk_gt = (int*)p;
  p += det_r256((size_t)n * DET_MAXB * 4);
  w.blk_eq = (int*)p;
  return w;
}

// Keys of slab k of one anchor for lane `sub` of its 16-lane group: key[j] belongs to class c0 + j.
// Multi-label: slab k covers classes 16 VEC k .. 16 VEC (k + 1) - 1, lane `sub` the VEC classes from
// (sub + 16 k) VEC, so lanes, then slabs, walk the classes in ascending order.  Best-class: one slab
// whose only key is the anchor's pick (best, bl) in lane 0 -- the arg-max first, the filter after.
template <int VEC, bool MULTI>
__device__ __forceinline__ void slab_keys(const DetArgs& d, const float* q, int sub, int k, float best, int bl,
                                          uint32_t (&key)[VEC], int& c0) {
  if (MULTI) {
    c0 = (sub + 16 * k) * VEC;
    float v[VEC];
    if (VEC == 4) {
      const float4 x = c0 < d.nc ? *reinterpret_cast<const float4*>(q + 4 + c0) : make_float4(0.f, 0.f, 0.f, 0.f);
      v[0] = x.x; v[VEC > 1 ? 1 : 0] = x.y; v[VEC > 2 ? 2 : 0] = x.z; v[VEC > 3 ? 3 : 0] = x.w;
    } else {
      v[0] = c0 < d.nc ? q[4 + c0] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      const int c = c0 + j;
      key[j] = (c < d.nc && v[j] > d.conf && (!d.mask || d.mask[c])) ? __float_as_uint(v[j]) : 0u;
    }
  } else {
    c0 = bl;
#pragma unroll
    for (int j = 0; j < VEC; ++j) key[j] = 0u;
    if (sub == 0 && best > d.conf && (!d.mask || d.mask[bl])) key[0] = __float_as_uint(best);
  }
}

template <int VEC, bool MULTI>
__device__ __forceinline__ int slab_count(int nc) {
  return MULTI ? (nc + 16 * VEC - 1) / (16 * VEC) : 1;
}

// sum over the block's 256 threads of two ints -> every thread (s_red: [2][4] ints of LDS)
__device__ __forceinline__ void block_sum2(int& a, int& b, int (*s_red)[4]) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    a += __shfl_xor(a, off);
    b += __shfl_xor(b, off);
  }
  const int wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { s_red[0][wv] = a; s_red[1][wv] = b; }
  __syncthreads();
  a = s_red[0][0] + s_red[0][1] + s_red[0][2] + s_red[0][3];
  b = s_red[1][0] + s_red[1][1] + s_red[1][2] + s_red[1][3];
  __syncthreads();
}

enum { DET_COUNT = 0, DET_HIST = 1, DET_RANK = 2 };

// grid (blocks per image, n).  COUNT: every image.  HIST (level 1 / 2) and RANK: overflowing images.
template <int VEC, bool MULTI, int MODE>
__global__ __launch_bounds__(256) void det_scan_kernel(DetArgs d, int level, DetWs w) {
  __shared__ uint32_t s_hist[MODE == DET_RANK ? 1 : DET_BINS];
  __shared__ int s_red[2][4];
  const int b = blockIdx.y, blk = blockIdx.x, n = gridDim.y;
  const uint32_t* st = w.state + 4 * (size_t)b;
  uint32_t ref = 0;                               // HIST: the prefix to match; RANK: the threshold key
  if (MODE != DET_COUNT) {
    if (st[0] == 0) return;                       // uniform for the block
    ref = st[1];
  }
  if (MODE != DET_RANK) {
    for (int i = threadIdx.x; i < DET_BINS; i += 256) s_hist[i] = 0;
    __syncthreads();
  }
  const int sub = threadIdx.x & 15, g = threadIdx.x >> 4;
  const int a_lo = blk * d.apb, a_hi = min(d.A, a_lo + d.apb);
  const int nslab = slab_count<VEC, MULTI>(d.nc);
  int gt = 0, eq = 0;
  for (int a = a_lo + g; a < a_hi; a += 16) {     // uniform for the 16-lane group
    const float* q = d.pred + ((size_t)b * d.A + a) * (4 + d.nc);
    float best = 0.f;
    int bl = 0;
    if (!MULTI) nms_pick16(q, d.nc, sub, best, bl);
    for (int k = 0; k < nslab; ++k) {
      uint32_t key[VEC];
      int c0;
      slab_keys<VEC, MULTI>(d, q, sub, k, best, bl, key, c0);
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        const uint32_t x = key[j];
        if (x == 0) continue;
        if (MODE == DET_COUNT) {
          ++gt;
          atomicAdd(&s_hist[x >> 20], 1u);
        } else if (MODE == DET_HIST) {
          if (level == 1) {
            if ((x >> 20) == ref) { atomicAdd(&s_hist[(x >> 9) & 2047u], 1u); ++gt; }
          } else {
            if ((x >> 9) == ref) { atomicAdd(&s_hist[x & 511u], 1u); ++gt; }
          }
        } else {
          gt += x > ref;
          eq += x == ref;
        }
      }
    }
  }
  block_sum2(gt, eq, s_red);                      // (also the barrier after the LDS atomics)
  if (MODE != DET_HIST && threadIdx.x == 0) {
    w.blk_gt[(size_t)b * DET_MAXB + blk] = gt;
    w.blk_eq[(size_t)b * DET_MAXB + blk] = eq;
    if (MODE == DET_COUNT && gt) atomicAdd(&w.total[b], (uint32_t)gt);
  }
  if (MODE != DET_RANK && gt) {                   // gt: the block's histogram entries
    uint32_t* h = w.hist + ((size_t)level * n + b) * DET_BINS;
    for (int i = threadIdx.x; i < DET_BINS; i += 256) {
      const uint32_t v = s_hist[i];
      if (v) atomicAdd(&h[i], v);
    }
  }
}

// One block per image: the bin of histogram `level` that holds the remaining-th key from the top.
__global__ __launch_bounds__(256) void det_select_kernel(int n, int K, int level, DetWs w) {
  __shared__ uint32_t s_sum[256];
  const int b = blockIdx.x;
  uint32_t* st = w.state + 4 * (size_t)b;
  if (level == 0) {
    if (w.total[b] <= (uint32_t)K) {
      if (threadIdx.x == 0) { st[0] = 0; st[1] = 0; st[2] = 0; st[3] = 0; }
      return;
    }
  } else if (st[0] == 0) {
    return;
  }
  const uint32_t* h = w.hist + ((size_t)level * n + b) * DET_BINS;
  uint32_t s = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) s += h[8 * threadIdx.x + i];
  s_sum[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t remaining = level == 0 ? (uint32_t)K : st[2];
    const uint32_t prefix = level == 0 ? 0u : st[1];
    uint32_t acc = 0;
    int t = 255;
    while (t > 0 && acc + s_sum[t] < remaining) { acc += s_sum[t]; --t; }
    int bin = 8 * t + 7;
    while (bin > 8 * t && acc + h[bin] < remaining) { acc += h[bin]; --bin; }
    st[0] = 1;
    st[1] = (prefix << (level == 2 ? 9 : 11)) | (uint32_t)bin;
    st[2] = remaining - acc;
    st[3] = 0;
  }
}

template <int VEC, bool MULTI>
__global__ __launch_bounds__(256) void det_write_kernel(DetArgs d, int K, DetWs w, float4* cand_boxes,
                                                        float* cand_score, int* cand_label, int* cand_anchor,
                                                        int* cand_count, int* cand_total) {
  __shared__ int s_red[2][4];
  __shared__ int s_g[16];
  const int b = blockIdx.y, blk = blockIdx.x;
  const uint32_t* st = w.state + 4 * (size_t)b;
  const uint32_t thr = st[1];
  const int quota = (int)st[2];
  const uint32_t T = w.total[b];
  const int cnt = (int)min(T, (uint32_t)K);
  // rows no candidate fills
  for (int r = cnt + blk * 256 + threadIdx.x; r < K; r += gridDim.x * 256) {
    const size_t o = (size_t)b * K + r;
    cand_boxes[o] = make_float4(0.f, 0.f, 0.f, 0.f);
    cand_score[o] = 0.f;
    cand_label[o] = -1;
    cand_anchor[o] = -1;
  }
  if (blk == 0 && threadIdx.x == 0) {
    cand_count[b] = cnt;
    cand_total[b] = (int)min(T, 0x7fffffffu);
  }
  // admitted-order offsets of this block: the sums over the image's earlier blocks
  int gt_base = (int)threadIdx.x < blk ? w.blk_gt[(size_t)b * DET_MAXB + threadIdx.x] : 0;
  int eq_base = (int)threadIdx.x < blk ? w.blk_eq[(size_t)b * DET_MAXB + threadIdx.x] : 0;
  block_sum2(gt_base, eq_base, s_red);
  const int sub = threadIdx.x & 15, g = threadIdx.x >> 4;
  const int a_lo = blk * d.apb, a_hi = min(d.A, a_lo + d.apb);
  const int nslab = slab_count<VEC, MULTI>(d.nc);
  for (int a0 = a_lo; a0 < a_hi; a0 += 16) {      // uniform for the block
    const int a = a0 + g;
    const bool valid = a < a_hi;                  // uniform for the 16-lane group
    const float* q = d.pred + ((size_t)b * d.A + (valid ? a : a_lo)) * (4 + d.nc);
    float best = 0.f;
    int bl = 0;
    if (!MULTI && valid) nms_pick16(q, d.nc, sub, best, bl);
    // the anchor's counts, packed (keys > thr) | (keys == thr) << 16: each at most nc <= 1024
    int mine = 0;
    if (valid) {
      for (int k = 0; k < nslab; ++k) {
        uint32_t key[VEC];
        int c0;
        slab_keys<VEC, MULTI>(d, q, sub, k, best, bl, key, c0);
#pragma unroll
        for (int j = 0; j < VEC; ++j)
          if (key[j]) mine += (key[j] > thr ? 1 : 0) + (key[j] == thr ? 0x10000 : 0);
      }
    }
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) mine += __shfl_xor(mine, off, 16);
    if (sub == 0) s_g[g] = mine;
    __syncthreads();
    int og = 0, oe = 0, tg = 0, te = 0;           // before this anchor in the round / the round's totals
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int v = s_g[i];
      tg += v & 0xffff;
      te += v >> 16;
      if (i < g) { og += v & 0xffff; oe += v >> 16; }
    }
    __syncthreads();
    if (valid && mine != 0) {
      int run_g = gt_base + og, run_e = eq_base + oe;
      const float4 box = nms_xyxy(q);
      for (int k = 0; k < nslab; ++k) {
        uint32_t key[VEC];
        int c0;
        slab_keys<VEC, MULTI>(d, q, sub, k, best, bl, key, c0);
        int lane = 0;
#pragma unroll
        for (int j = 0; j < VEC; ++j)
          if (key[j]) lane += (key[j] > thr ? 1 : 0) + (key[j] == thr ? 0x10000 : 0);
        int inc = lane;                           // inclusive scan over the 16 lanes
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
          const int y = __shfl_up(inc, o, 16);
          if (sub >= o) inc += y;
        }
        const int tot = __shfl(inc, 15, 16);
        int my_g = run_g + ((inc - lane) & 0xffff), my_e = run_e + ((inc - lane) >> 16);
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          const uint32_t x = key[j];
          if (x == 0) continue;
          const bool is_gt = x > thr, is_eq = x == thr;
          if (is_gt || (is_eq && my_e < quota)) {
            const int row = my_g + min(my_e, quota);
            if (row < K) {
              const size_t o = (size_t)b * K + row;
              cand_boxes[o] = box;
              cand_score[o] = __uint_as_float(x);
              cand_label[o] = c0 + j;
              cand_anchor[o] = a;
            }
          }
          my_g += is_gt;
          my_e += is_eq;
        }
        run_g += tot & 0xffff;
        run_e += tot >> 16;
      }
    }
    gt_base += tg;
    eq_base += te;
  }
}

// ---------------------------------------------------------------------------------------
// finalize
// ---------------------------------------------------------------------------------------
// VOTE: the box slot of an emitted row carries its candidate row id (int bits in o[0]) to det_vote_kernel.
template <bool VOTE>
__global__ __launch_bounds__(1024) void det_finalize_kernel(int K, int max_det, const float4* cand_boxes,
                                                            const float* cand_score, const int* true_label,
                                                            const int* cand_anchor, const int64_t* keep_idx,
                                                            const int* counts, const float* frames, float* det,
                                                            int* det_anchor, int* det_count) {
  __shared__ uint32_t s_hist[DET_BINS];
  __shared__ uint32_t s_sum[64];
  __shared__ uint64_t s_key[DET_MAX_DET];
  __shared__ uint64_t s_sel[2];                   // prefix, remaining
  __shared__ int s_n;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int cnt = min(max(counts[b], 0), K);
  const int64_t* kp = keep_idx + (size_t)b * K;
  const float* sc = cand_score + (size_t)b * K;
  // a kept row's key: score bits (positive floats order as integers), then the lower row first; unique
  auto key_of = [&](int i) -> uint64_t {
    const int64_t r = kp[i];
    if (r < 0 || r >= K) return 0;
    return ((uint64_t)(__float_as_uint(sc[r]) & 0x7fffffffu) << 17) | (uint64_t)(0x1ffff - (int)r);
  };
  uint64_t thr = 1;                               // every valid key
  if (cnt > max_det) {                            // radix select of the max_det-th key, 48 bits top down
    if (tid == 0) { s_sel[0] = 0; s_sel[1] = (uint64_t)max_det; }
    for (int level = 0; level < 5; ++level) {
      const int shift = level < 4 ? 37 - 11 * level : 0;      // digits at bits 47..37, 36..26, 25..15, 14..4, 3..0
      const int width = level < 4 ? 11 : 4;
      for (int i = tid; i < DET_BINS; i += 1024) s_hist[i] = 0;
      __syncthreads();
      const uint64_t prefix = s_sel[0];
      for (int i = tid; i < cnt; i += 1024) {
        const uint64_t x = key_of(i);
        if (x != 0 && (x >> (shift + width)) == prefix)
          atomicAdd(&s_hist[(uint32_t)(x >> shift) & ((1u << width) - 1u)], 1u);
      }
      __syncthreads();
      if (tid < 64) {
        uint32_t s = 0;
        for (int i = 0; i < 32; ++i) s += s_hist[32 * tid + i];
        s_sum[tid] = s;
      }
      __syncthreads();
      if (tid == 0) {
        const uint64_t remaining = s_sel[1];
        uint64_t acc = 0;
        int t = 63;
        while (t > 0 && acc + s_sum[t] < remaining) { acc += s_sum[t]; --t; }
        int bin = 32 * t + 31;
        while (bin > 32 * t && acc + s_hist[bin] < remaining) { acc += s_hist[bin]; --bin; }
        s_sel[0] = (prefix << width) | (uint64_t)bin;
        s_sel[1] = remaining - acc;
      }
      __syncthreads();
    }
    thr = s_sel[0];
  }
  if (tid == 0) s_n = 0;
  s_key[tid] = 0;
  __syncthreads();
  for (int i = tid; i < cnt; i += 1024) {
    const uint64_t x = key_of(i);
    if (x != 0 && x >= thr) {
      const int slot = atomicAdd(&s_n, 1);        // the slot order does not matter: sorted below
      if (slot < DET_MAX_DET) s_key[slot] = x;
    }
  }
  __syncthreads();
  const int m = min(s_n, max_det);
  // bitonic sort, descending (keys are unique; the padding is 0, below every key)
  for (int k = 2; k <= DET_MAX_DET; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      const int ixj = tid ^ j;
      if (ixj > tid) {
        const uint64_t x = s_key[tid], y = s_key[ixj];
        if ((tid & k) == 0 ? x < y : x > y) { s_key[tid] = y; s_key[ixj] = x; }
      }
      __syncthreads();
    }
  }
  if (tid == 0) det_count[b] = m;
  if (tid < max_det) {
    float* o = det + ((size_t)b * max_det + tid) * 6;
    if (tid < m) {
      const int r = 0x1ffff - (int)(s_key[tid] & 0x1ffffu);
      float4 q = VOTE ? make_float4(0.f, 0.f, 0.f, 0.f) : cand_boxes[(size_t)b * K + r];
      if (!VOTE && frames) {
        const float* f = frames + 6 * (size_t)b;  // gain_x, gain_y, pad_x, pad_y, w0, h0
        q.x = fminf(fmaxf((q.x - f[2]) / f[0], 0.f), f[4]);
        q.y = fminf(fmaxf((q.y - f[3]) / f[1], 0.f), f[5]);
        q.z = fminf(fmaxf((q.z - f[2]) / f[0], 0.f), f[4]);
        q.w = fminf(fmaxf((q.w - f[3]) / f[1], 0.f), f[5]);
      }
      o[0] = q.x; o[1] = q.y; o[2] = q.z; o[3] = q.w;
      if (VOTE) reinterpret_cast<int*>(o)[0] = r;
      o[4] = sc[r];
      o[5] = (float)true_label[(size_t)b * K + r];
      det_anchor[(size_t)b * max_det + tid] = cand_anchor[(size_t)b * K + r];
    } else {
      o[0] = 0.f; o[1] = 0.f; o[2] = 0.f; o[3] = 0.f; o[4] = 0.f;
      o[5] = -1.f;
      det_anchor[(size_t)b * max_det + tid] = -1;
    }
  }
}

// One wavefront per emitted detection (b, i), 4 per block: grid (ceil(max_det / 4), n).  Row r of the
// detection comes from det_finalize_kernel<true>; the members are the live rows j < cand_count[b] with
// r's NMS label and iou_gt(r, j).  Sums in float64 (lane-strided, then a xor-shuffle tree: a fixed
// order), one rounding to fp32.  A score sum that is 0 (no member: a zero-area box's overlap with
// itself is NaN) or not finite (+inf score) leaves the row its own box.
__global__ __launch_bounds__(256) void det_vote_kernel(int K, int max_det, const float4* cand_boxes,
                                                       const float* cand_score, const int* nms_label,
                                                       const int* cand_count, double iou, const float* frames,
                                                       float* det, const int* det_count) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);          // uniform for the wavefront
  if (i >= max_det || i >= det_count[b]) return;
  float* o = det + ((size_t)b * max_det + i) * 6;
  const int r = reinterpret_cast<const int*>(o)[0];
  if (r < 0 || r >= K) return;
  const int cnt = min(max(cand_count[b], 0), K);
  const float4* bx = cand_boxes + (size_t)b * K;
  const float* sc = cand_score + (size_t)b * K;
  const int* lb = nms_label + (size_t)b * K;
  const float4 bi = bx[r];
  const int li = lb[r];
  double sw = 0.0, s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  for (int j = lane; j < cnt; j += 64) {
    if (lb[j] != li) continue;
    const float4 bj = bx[j];
    if (!iou_gt(bi, bj, iou)) continue;
    const double w = (double)sc[j];
    sw += w;
    s0 += w * (double)bj.x;
    s1 += w * (double)bj.y;
    s2 += w * (double)bj.z;
    s3 += w * (double)bj.w;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    sw += __shfl_xor(sw, off);
    s0 += __shfl_xor(s0, off);
    s1 += __shfl_xor(s1, off);
    s2 += __shfl_xor(s2, off);
    s3 += __shfl_xor(s3, off);
  }
  if (lane != 0) return;
  float4 q = bi;
  if (sw != 0.0 && isfinite(sw)) q = make_float4((float)(s0 / sw), (float)(s1 / sw), (float)(s2 / sw), (float)(s3 / sw));
  if (frames) {
    const float* f = frames + 6 * (size_t)b;
    q.x = fminf(fmaxf((q.x - f[2]) / f[0], 0.f), f[4]);
    q.y = fminf(fmaxf((q.y - f[3]) / f[1], 0.f), f[5]);
    q.z = fminf(fmaxf((q.z - f[2]) / f[0], 0.f), f[4]);
    q.w = fminf(fmaxf((q.w - f[3]) / f[1], 0.f), f[5]);
  }
  o[0] = q.x; o[1] = q.y; o[2] = q.z; o[3] = q.w;
}

}  // namespace yms

using namespace yms;

extern "C" {

size_t yms_det_ws_bytes(int n, int A, int nc, int K) {
  if (n <= 0 || A <= 0 || nc <= 0 || K <= 0) return 0;
  return det_ws_bytes(n);
}

yms_status yms_det_candidates(int n, int A, int nc, const float* pred, float conf, int multi_label,
                              const uint8_t* class_mask, int K, float* cand_boxes, float* cand_score,
                              int* cand_label, int* cand_anchor, int* cand_count, int* cand_total, void* ws,
                              size_t ws_bytes, void* stream) {
  if (n <= 0 || n > 65535 || A <= 0 || nc <= 0 || nc > 1024 || (long)A * nc > 0x7fffffffL) return YMS_ERR_INVALID;
  if (!pred || !cand_boxes || !cand_score || !cand_label || !cand_anchor || !cand_count || !cand_total || !ws)
    return YMS_ERR_INVALID;
  if (!(conf >= 0.0f)) return YMS_ERR_INVALID;    // negative or NaN: keys would not order as integers
  if (K < 1 || K > DET_MAX_K) return YMS_ERR_INVALID;
  if (ws_bytes < det_ws_bytes(n)) return YMS_ERR_INVALID;
  if ((uintptr_t)ws % 16 != 0 || (uintptr_t)cand_boxes % 16 != 0 || (uintptr_t)pred % 4 != 0) return YMS_ERR_INVALID;
  hipStream_t st = (hipStream_t)stream;
  DetWs w = det_carve(ws, n);
  DetArgs d;
  d.A = A;
  d.nc = nc;
  d.apb = (int)rup(std::max(32, cdiv(A, DET_MAXB)), 16);
  d.pred = pred;
  d.conf = conf;
  d.mask = class_mask;
  const dim3 grid((unsigned)cdiv(A, d.apb), (unsigned)n), blk(256);
  if (hipMemsetAsync(w.hist, 0, ((size_t)3 * n * DET_BINS + n) * 4, st) != hipSuccess) return YMS_ERR_LAUNCH;
  const int variant = !multi_label ? 2 : (nc % 4 == 0 && (uintptr_t)pred % 16 == 0) ? 0 : 1;
#define DET_SCAN(MODE, level)                                                                             \
  do {                                                                                                    \
    if (variant == 0) hipLaunchKernelGGL((det_scan_kernel<4, true, MODE>), grid, blk, 0, st, d, level, w); \
    else if (variant == 1) hipLaunchKernelGGL((det_scan_kernel<1, true, MODE>), grid, blk, 0, st, d, level, w); \
    else hipLaunchKernelGGL((det_scan_kernel<1, false, MODE>), grid, blk, 0, st, d, level, w);            \
  } while (0)
  DET_SCAN(DET_COUNT, 0);
  hipLaunchKernelGGL(det_select_kernel, dim3((unsigned)n), blk, 0, st, n, K, 0, w);
  DET_SCAN(DET_HIST, 1);
  hipLaunchKernelGGL(det_select_kernel, dim3((unsigned)n), blk, 0, st, n, K, 1, w);
  DET_SCAN(DET_HIST, 2);
  hipLaunchKernelGGL(det_select_kernel, dim3((unsigned)n), blk, 0, st, n, K, 2, w);
  DET_SCAN(DET_RANK, 0);
#undef DET_SCAN
  float4* cb = reinterpret_cast<float4*>(cand_boxes);
  if (variant == 0)
    hipLaunchKernelGGL((det_write_kernel<4, true>), grid, blk, 0, st, d, K, w, cb, cand_score, cand_label, cand_anchor,
                       cand_count, cand_total);
  else if (variant == 1)
    hipLaunchKernelGGL((det_write_kernel<1, true>), grid, blk, 0, st, d, K, w, cb, cand_score, cand_label, cand_anchor,
                       cand_count, cand_total);
  else
    hipLaunchKernelGGL((det_write_kernel<1, false>), grid, blk, 0, st, d, K, w, cb, cand_score, cand_label,
                       cand_anchor, cand_count, cand_total);
  return launch_status();
}

yms_status yms_det_finalize(int n, int K, int max_det, const float* cand_boxes, const float* cand_score,
                            const int* true_label, const int* cand_anchor, const int64_t* keep_idx,
                            const int* counts, const float* frames, float* det, int* det_anchor, int* det_count,
                            void* stream) {
  if (n <= 0 || K < 1 || K > DET_MAX_K || max_det < 1 || max_det > DET_MAX_DET) return YMS_ERR_INVALID;
  if (!cand_boxes || !cand_score || !true_label || !cand_anchor || !keep_idx || !counts || !det || !det_anchor ||
      !det_count)
    return YMS_ERR_INVALID;
  if ((uintptr_t)cand_boxes % 16 != 0) return YMS_ERR_INVALID;
  hipLaunchKernelGGL(det_finalize_kernel<false>, dim3((unsigned)n), dim3(1024), 0, (hipStream_t)stream, K, max_det,
                     reinterpret_cast<const float4*>(cand_boxes), cand_score, true_label, cand_anchor, keep_idx,
                     counts, frames, det, det_anchor, det_count);
  return launch_status();
}

yms_status yms_det_finalize_vote(int n, int K, int max_det, const float* cand_boxes, const float* cand_score,
                                 const int* true_label, const int* cand_anchor, const int64_t* keep_idx,
                                 const int* counts, const float* frames, const int* cand_count,
                                 const int* nms_label, double iou, float* det, int* det_anchor, int* det_count,
                                 void* stream) {
  if (n <= 0 || n > 65535 || K < 1 || K > DET_MAX_K || max_det < 1 || max_det > DET_MAX_DET) return YMS_ERR_INVALID;
  if (!cand_boxes || !cand_score || !true_label || !cand_anchor || !keep_idx || !counts || !cand_count ||
      !nms_label || !det || !det_anchor || !det_count)
    return YMS_ERR_INVALID;
  if ((uintptr_t)cand_boxes % 16 != 0 || iou != iou) return YMS_ERR_INVALID;
  hipStream_t st = (hipStream_t)stream;
  const float4* cb = reinterpret_cast<const float4*>(cand_boxes);
  hipLaunchKernelGGL(det_finalize_kernel<true>, dim3((unsigned)n), dim3(1024), 0, st, K, max_det, cb, cand_score,
                     true_label, cand_anchor, keep_idx, counts, frames, det, det_anchor, det_count);
  hipLaunchKernelGGL(det_vote_kernel, dim3((unsigned)cdiv(max_det, 4), (unsigned)n), dim3(256), 0, st, K, max_det,
                     cb, cand_score, nms_label, cand_count, iou, frames, det, det_count);
  return launch_status();
}

}  // extern "C"
