// mAP@0.5 evaluation: GPU per-image detection <-> ground-truth matching and the
// host-side per-class precision/recall accumulation, replacing the reference's
// torchmetrics.MeanAveragePrecision(iou_thresholds=[0.5]) call in validate_epoch
// (yolov8/tools/train.py:41-47, 146, 152-153).  The semantics are the published COCOeval
// algorithm at that setting (oracle/map_ref.py restates it; torchmetrics / pycocotools are not
// installed here, so parity is against that restatement):
//   per (image, class): detections stably sorted by score (descending), the first 100 kept;
//   greedy matching in that order at IoU >= 0.5 (double precision, xywh areas, no +1), each
//   detection taking the unmatched ground truth of highest IoU (ties -> the later one);
//   per class: kept detections ordered by (score desc, image, input index), tp/fp cumsums,
//   precision made monotone, 101-point interpolation; mAP = mean over classes with ground truth.
// COCO AP (mAP@[.5:.95], AP by object size, AR@1/10/100): map_match_coco_kernel runs the same matching
// for up to 16 IoU thresholds x the four COCOeval area ranges at once, one (threshold, area) pair per
// lane, with COCOeval's ignore rules (out-of-range ground truths are visited last and only taken when
// no in-range one qualifies; a detection matched to one, or unmatched and itself out of range, is
// ignored); yms_map_accumulate_coco fills COCOeval's precision / recall tables on the host.  The _gt entry
// points add COCOeval's two per-annotation fields: iscrowd (a crowd ground truth is ignore in every range,
// scored as intersection / detection area, and may be matched by any number of detections) and area (the
// annotation's own area decides its size class instead of w*h).
// map_match_coco_fixed_kernel is the same matching on yms.ops.detect's padded layout, written into the
// epoch buffers that csrc/map_accum.hip accumulates on the device.
#include <algorithm>
#include <cmath>
#include <vector>

#include "yms_common.hpp"

namespace yms {

constexpr int MAP_MAXDET = 100;
constexpr int MAP_MAX_GT = 2048;      // ground truths per image (LDS)

// one wave per image
__global__ __launch_bounds__(64) void map_match_kernel(const float* dbox, const float* dscore, const int* dlabel,
                                                       const int* doff, const float* gbox, const int* glabel,
                                                       const int* goff, uint8_t* tp, uint8_t* kept, int* rank_out) {
  __shared__ double gb[MAP_MAX_GT][4];
  __shared__ int gl[MAP_MAX_GT];
  __shared__ uint8_t gm[MAP_MAX_GT];
  const int img = blockIdx.x, lane = threadIdx.x;
  const int d0 = doff[img], nd = doff[img + 1] - d0;
  const int g0 = goff[img], ng = goff[img + 1] - g0;
  for (int j = lane; j < ng; j += 64) {
    const float* q = gbox + (long)(g0 + j) * 4;
    gb[j][0] = (double)q[0];
    gb[j][1] = (double)q[1];
    gb[j][2] = (double)(q[2] - q[0]);     // width / height in fp32, as box_convert
    gb[j][3] = (double)(q[3] - q[1]);
    gl[j] = glabel[g0 + j];
    gm[j] = 0;
  }
  // rank of every detection within its class: stable descending score order
  for (int d = lane; d < nd; d += 64) {
    const int lab = dlabel[d0 + d];
    const float sc = dscore[d0 + d];
    int r = 0;
    for (int j = 0; j < nd; ++j) {
      if (dlabel[d0 + j] != lab) continue;
      const float sj = dscore[d0 + j];
      r += (sj > sc || (sj == sc && j < d)) ? 1 : 0;
    }
    rank_out[d0 + d] = r;
    kept[d0 + d] = r < MAP_MAXDET ? 1 : 0;
    tp[d0 + d] = 0;
  }
  __syncthreads();
  // greedy matching per ground-truth class, detections in rank order
  for (int gi = 0; gi < ng; ++gi) {
    const int c = gl[gi];
    bool first = true;                     // process each class once: at its first ground truth
    for (int j = 0; j < gi; ++j)
      if (gl[j] == c) { first = false; break; }
    if (!first) continue;
    for (int r = 0; r < MAP_MAXDET; ++r) {
      // the class-c detection of rank r (at most one)
      int found = -1;
      for (int d = lane; d < nd; d += 64)
        if (dlabel[d0 + d] == c && rank_out[d0 + d] == r) found = d;
      unsigned long long any = __ballot(found >= 0);
      if (!any) break;                    // fewer than r + 1 detections of this class
      const int src = __ffsll((long long)any) - 1;
      const int d = __shfl(found, src);
      // xyxy -> xywh in fp32 (torchvision box_convert on the fp32 tensors), IoU in double
      const float* bp = dbox + (long)(d0 + d) * 4;
      const double b[2] = {(double)bp[0], (double)bp[1]};
      const double bw = (double)(bp[2] - bp[0]), bh = (double)(bp[3] - bp[1]);
      // best unmatched ground truth: max IoU >= 0.5, the later index on ties
      double best = -1.0;
      int bj = -1;
      for (int j = lane; j < ng; j += 64) {
        if (gl[j] != c || gm[j]) continue;
        const double gw = gb[j][2], gh = gb[j][3];
        const double w = fmin(b[0] + bw, gb[j][0] + gw) - fmax(b[0], gb[j][0]);
        const double h = fmin(b[1] + bh, gb[j][1] + gh) - fmax(b[1], gb[j][1]);
        double iou = 0.0;
        if (w > 0.0 && h > 0.0) {
          const double inter = w * h;
          iou = inter / (bw * bh + gw * gh - inter);
        }
        if (iou >= fmin(0.5, 1.0 - 1e-10) && (iou > best || (iou == best && j > bj))) {
          best = iou;
          bj = j;
        }
      }
#pragma unroll
      for (int m = 1; m < 64; m <<= 1) {
        const double ob = __shfl_xor(best, m);
        const int oj = __shfl_xor(bj, m);
        if (ob > best || (ob == best && oj > bj)) {
          best = ob;
          bj = oj;
        }
      }
      if (bj >= 0) {
        if (lane == 0) {
          gm[bj] = 1;
          tp[d0 + d] = 1;
        }
      }
      __syncthreads();
    }
  }
}

// ---- COCO matching: T thresholds x 4 area ranges ------------------------------------------------
constexpr int MAP_MAX_THR = 16;
constexpr int MAP_N_AREA = 4;
constexpr int MAP_COCO_WAVES = 4;
constexpr int MAP_FIXED_MAX_DET = 1024;      // padded rows per image (yms.ops.detect's max_det limit)
constexpr int MAP_MAX_CLASSES = 4096;

struct MapCocoThr {
  double thr[MAP_MAX_THR];
  int n;
};

// COCOeval's areaRng all / small / medium / large, both ends inclusive: bit a set = out of range a
__device__ __forceinline__ unsigned map_area_out_bits(double area) {
  unsigned b = 0;
  if (area < 0.0 || area > 1e10) b |= 1u;
  if (area < 0.0 || area > 1024.0) b |= 2u;
  if (area < 1024.0 || area > 9216.0) b |= 4u;
  if (area < 9216.0 || area > 1e10) b |= 8u;
  return b;
}

// gig[] bit 4: the ground truth is a crowd (bits 0..3: out of area range a)
constexpr unsigned MAP_GT_CROWD = 16u;

// maskUtils.iou on xywh doubles, every product and sum rounded on its own as numpy does; against a crowd
// ground truth the union is the detection's own area (intersection over detection area)
__device__ __forceinline__ double map_iou_xywh(double bx, double by, double bw, double bh, double gx, double gy,
                                               double gw, double gh, bool crowd) {
#pragma clang fp contract(off)
  const double w = fmin(bx + bw, gx + gw) - fmax(bx, gx);
  const double h = fmin(by + bh, gy + gh) - fmax(by, gy);
  if (!(w > 0.0 && h > 0.0)) return 0.0;
  const double inter = w * h;
  const double a = bw * bh, b = gw * gh;
  return inter / (crowd ? a : a + b - inter);
}

// One workgroup (4 waves) per image.  Setup: the image's ground truths are staged in LDS as xywh
// doubles ordered by (class, input index), so a class is one contiguous segment in COCOeval's
// visiting order; detections are ranked within their class and listed by (class, rank) in order_ws.
// Matching: the waves take the image's ground-truth classes in turn; lane = area * 16 + threshold
// runs its own greedy matching over the class's <= 100 kept detections.  Per detection the wave
// computes the IoUs against the segment 64 ground truths at a time and broadcasts only those that
// reach the lowest threshold; each lane keeps the best unmatched in-range and out-of-range candidate
// (later one on ties) and takes the in-range one if there is any (COCOeval's break).  The "already
// matched" bits are one LDS word column per lane (gm[wave][word][lane]): no lane shares a word, and
// classes own disjoint bits, so they are cleared once.  There is no barrier after the setup.
// GT = the per-ground-truth fields of COCOeval's evaluateImg / computeIoU are given (gt_crowd, gt_area: each
// may still be null on its own; with GT = false neither is read and the code is the one without them):
//   area ranges: a ground truth's range bits come from (double)gt_area[j] when given, else from w*h; the
//     comparisons are map_area_out_bits' (a negative area is out of every range, a NaN inside every one);
//   crowd as ignore: gt_crowd[j] != 0 makes the ground truth ignore in all four ranges.  It stays at its
//     (class, input index) place, so crowd and out-of-range ground truths interleave by input index as in
//     COCOeval's stable sort on the ignore flag, and the "later one on ties" rule covers both;
//   crowd IoU: intersection / detection area (map_iou_xywh's crowd form);
//   repeated matching: the "already matched" test is skipped for a crowd, so any number of detections can
//     take the same one; a detection whose best candidate is a crowd is matched and ignored; an in-range
//     match still wins over any ignored one.
// The crowd flag is bit 4 of gig[]; gt_area is only read during the setup.
// The body is shared by the two layouts (prefix offsets / padded rows): every pointer is the image's
// own first detection / ground truth, nd / ng its counts, mstride the masks' area stride.
template <bool GT>
__device__ __forceinline__ void map_match_coco_image(const float* dbox, const float* dscore, const int* dlabel,
                                                     int nd, const float* gbox, const int* glabel,
                                                     const uint8_t* gt_crowd, const float* gt_area, int ng,
                                                     const MapCocoThr& P, long mstride, uint16_t* dmatch,
                                                     uint16_t* dign, uint8_t* gign_out, int* rank_out,
                                                     int* order_ws) {
  __shared__ double gb[MAP_MAX_GT][4];
  __shared__ int gl[MAP_MAX_GT];
  __shared__ int heads[MAP_MAX_GT];
  __shared__ uint8_t gig[MAP_MAX_GT];
  __shared__ unsigned gm[MAP_COCO_WAVES][MAP_MAX_GT / 32][64];
  __shared__ int n_heads;
  static_assert(sizeof(gb) + sizeof(gl) + sizeof(heads) + sizeof(gig) + sizeof(gm) + sizeof(int) <= 160 * 1024,
                "the matching's LDS arrays must fit one workgroup's 160 KB");
  constexpr int NT = 64 * MAP_COCO_WAVES;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (ng > MAP_MAX_GT) return;            // the host entry point refuses these; never index past the LDS arrays
  const int T = P.n;
  const unsigned tmask = (1u << T) - 1u;
  if (tid == 0) n_heads = 0;
  // ground truths -> LDS in (class, input index) order, with their area-ignore bits
  for (int j = tid; j < ng; j += NT) {
    const int lab = glabel[j];
    int p = 0;
    for (int i = 0; i < ng; ++i) {
      const int li = glabel[i];
      p += (li < lab || (li == lab && i < j)) ? 1 : 0;
    }
    const float* q = gbox + (long)j * 4;
    const double gw = (double)(q[2] - q[0]), gh = (double)(q[3] - q[1]);   // width / height in fp32, as box_convert
    gb[p][0] = (double)q[0];
    gb[p][1] = (double)q[1];
    gb[p][2] = gw;
    gb[p][3] = gh;
    gl[p] = lab;
    unsigned bits = map_area_out_bits(GT && gt_area ? (double)gt_area[j] : gw * gh);
    if (GT && gt_crowd && gt_crowd[j]) bits = MAP_GT_CROWD | 15u;
    gig[p] = (uint8_t)bits;
    if (gign_out) gign_out[j] = (uint8_t)(bits & 15u);
  }
  for (int w = 0; w < (ng + 31) / 32; ++w) gm[wave][w][lane] = 0u;
  // detections: rank within the class (stable descending score), position in (class, rank) order,
  // and the masks of an unmatched detection (classes without ground truth here keep them)
  for (int d = tid; d < nd; d += NT) {
    const int lab = dlabel[d];
    const float sc = dscore[d];
    int r = 0, below = 0;
    for (int j = 0; j < nd; ++j) {
      const int lj = dlabel[j];
      below += lj < lab ? 1 : 0;
      if (lj != lab) continue;
      const float sj = dscore[j];
      r += (sj > sc || (sj == sc && j < d)) ? 1 : 0;
    }
    rank_out[d] = r;
    order_ws[below + r] = d;
    const float* bp = dbox + (long)d * 4;
    const unsigned out = map_area_out_bits((double)(bp[2] - bp[0]) * (double)(bp[3] - bp[1]));
#pragma unroll
    for (int a = 0; a < MAP_N_AREA; ++a) {
      dmatch[a * mstride + d] = 0;
      dign[a * mstride + d] = (uint16_t)(((out >> a) & 1u) ? tmask : 0u);
    }
  }
  __syncthreads();
  for (int p = tid; p < ng; p += NT)
    if (p == 0 || gl[p] != gl[p - 1]) heads[atomicAdd(&n_heads, 1)] = p;
  __syncthreads();
  const int nh = n_heads;

  const int t = lane & 15, a = lane >> 4;
  const bool live = t < T;
  const double thr_l = fmin(P.thr[live ? t : 0], 1.0 - 1e-10);
  const double thr_min = fmin(P.thr[0], 1.0 - 1e-10);      // thresholds are increasing
  for (int h = wave; h < nh; h += MAP_COCO_WAVES) {
    const int gs = heads[h], c = gl[gs];
    int gn = 0;
    for (int base = gs; base < ng; base += 64) {
      const unsigned long long same = __ballot(base + lane < ng && gl[min(base + lane, ng - 1)] == c);
      gn += __popcll(same);
      if (same != ~0ull) break;
    }
    int ds = 0, dn = 0;
    for (int base = 0; base < nd; base += 64) {
      const int lj = base + lane < nd ? dlabel[base + lane] : 0x7fffffff;
      ds += __popcll(__ballot(lj < c));
      dn += __popcll(__ballot(lj == c));
    }
    const int nr = min(dn, MAP_MAXDET);
    for (int r = 0; r < nr; ++r) {
      const int d = order_ws[ds + r];
      if ((unsigned)d >= (unsigned)nd) continue;      // NaN scores leave holes in the order: never index by one
      const float* bp = dbox + (long)d * 4;
      const double bx = (double)bp[0], by = (double)bp[1];
      const double bw = (double)(bp[2] - bp[0]), bh = (double)(bp[3] - bp[1]);
      const bool d_out = (map_area_out_bits(bw * bh) >> a) & 1u;
      double best_n = thr_l, best_i = thr_l;      // in-range / out-of-range (ignored) ground truths
      int jn = -1, ji = -1;
      for (int base = 0; base < gn; base += 64) {
        const int p = gs + base + lane;
        double iou = 0.0;
        if (base + lane < gn)
          iou = map_iou_xywh(bx, by, bw, bh, gb[p][0], gb[p][1], gb[p][2], gb[p][3], GT && (gig[p] & MAP_GT_CROWD));
        unsigned long long cand = __ballot(base + lane < gn && iou >= thr_min);
        while (cand) {                                 // wave-uniform: candidates in visiting order
          const int src = __ffsll((long long)cand) - 1;
          cand &= cand - 1;
          const double ci = __shfl(iou, src);
          const int cp = gs + base + src;
          const bool crowd = GT && (gig[cp] & MAP_GT_CROWD);      // cp is uniform: a crowd is never used up
          if (!live || (!crowd && ((gm[wave][cp >> 5][lane] >> (cp & 31)) & 1u))) continue;
          if ((gig[cp] >> a) & 1u) {
            if (ci >= best_i) { best_i = ci; ji = cp; }
          } else {
            if (ci >= best_n) { best_n = ci; jn = cp; }
          }
        }
      }
      const int m = jn >= 0 ? jn : ji;
      const bool matched = live && m >= 0;
      if (matched) gm[wave][m >> 5][lane] |= 1u << (m & 31);
      const bool ign = live && (matched ? jn < 0 : d_out);
      const unsigned long long bm = __ballot(matched), bi = __ballot(ign);
      if (lane < MAP_N_AREA) {
        dmatch[lane * mstride + d] = (uint16_t)((bm >> (16 * lane)) & 0xffffull);
        dign[lane * mstride + d] = (uint16_t)((bi >> (16 * lane)) & 0xffffull);
      }
    }
  }
}

template <bool GT>
__global__ __launch_bounds__(64 * MAP_COCO_WAVES) void map_match_coco_kernel(
    const float* dbox, const float* dscore, const int* dlabel, const int* doff, const float* gbox, const int* glabel,
    const uint8_t* gt_crowd, const float* gt_area, const int* goff, MapCocoThr P, long n_det, uint16_t* dmatch,
    uint16_t* dign, uint8_t* gign_out, int* rank_out, int* order_ws) {
  const int img = blockIdx.x;
  const int d0 = doff[img], nd = doff[img + 1] - d0;
  const int g0 = goff[img], ng = goff[img + 1] - g0;
  map_match_coco_image<GT>(dbox + (long)d0 * 4, dscore + d0, dlabel + d0, nd, gbox + (long)g0 * 4, glabel + g0,
                           GT && gt_crowd ? gt_crowd + g0 : nullptr, GT && gt_area ? gt_area + g0 : nullptr, ng, P,
                           n_det, dmatch + d0, dign + d0, gign_out + g0, rank_out + d0, order_ws + d0);
}

// The padded layout of yms.ops.detect: image i owns rows [i * max_det, (i + 1) * max_det) of the inputs and
// rows row0 + the same of the epoch buffers (masks: area stride cap).  Counts are read on the device and
// clamped to the padded widths.  Every owned row is written: dead rows (slot >= count) get score 0, label -1,
// rank -1 and zero masks; live rows the shared matching's results plus a copy of their score and label.
// npig[class][area] += the image's ground truths that are in range (integer atomics): never a crowd, and by
// gt_area where it is given.
template <bool GT>
__global__ __launch_bounds__(64 * MAP_COCO_WAVES) void map_match_coco_fixed_kernel(
    const float* dbox, const float* dscore, const int* dlabel, const int* dcount, int max_det, const float* gbox,
    const int* glabel, const uint8_t* gt_crowd, const float* gt_area, const int* gcount, int max_gt, MapCocoThr P,
    int n_classes, long cap, long row0, float* score, int* label, int* rank_out, uint16_t* dmatch, uint16_t* dign,
    int* npig, int* order_ws) {
  constexpr int NT = 64 * MAP_COCO_WAVES;
  const int img = blockIdx.x, tid = threadIdx.x;
  const int nd = min(max(dcount[img], 0), max_det);
  const int ng = min(max(gcount[img], 0), max_gt);
  const long in0 = (long)img * max_det, out0 = row0 + in0, gin0 = (long)img * max_gt;
  for (int d = tid; d < max_det; d += NT) {
    const bool on = d < nd;
    score[out0 + d] = on ? dscore[in0 + d] : 0.0f;
    label[out0 + d] = on ? dlabel[in0 + d] : -1;
    if (!on) {
      rank_out[out0 + d] = -1;
#pragma unroll
      for (int a = 0; a < MAP_N_AREA; ++a) {
        dmatch[a * cap + out0 + d] = 0;
        dign[a * cap + out0 + d] = 0;
      }
    }
  }
  for (int j = tid; j < ng; j += NT) {
    const int lab = glabel[gin0 + j];
    if (lab < 0 || lab >= n_classes) continue;
    if (GT && gt_crowd && gt_crowd[gin0 + j]) continue;
    const float* q = gbox + (gin0 + j) * 4;
    const unsigned bits = map_area_out_bits(GT && gt_area ? (double)gt_area[gin0 + j]
                                                          : (double)(q[2] - q[0]) * (double)(q[3] - q[1]));
#pragma unroll
    for (int a = 0; a < MAP_N_AREA; ++a)
      if (!((bits >> a) & 1u)) atomicAdd(&npig[lab * MAP_N_AREA + a], 1);
  }
  map_match_coco_image<GT>(dbox + in0 * 4, dscore + in0, dlabel + in0, nd, gbox + gin0 * 4, glabel + gin0,
                           GT && gt_crowd ? gt_crowd + gin0 : nullptr, GT && gt_area ? gt_area + gin0 : nullptr, ng,
                           P, cap, dmatch + out0, dign + out0, nullptr, rank_out + out0, order_ws + in0);
}

}  // namespace yms

using namespace yms;

// numpy's pairwise summation (np.mean / np.sum over float64 arrays), so the host AP matches the
// COCOeval restatement bit for bit
static double np_pairwise_sum(const double* a, long n) {
  if (n < 8) {
    double r = 0.0;
    for (long i = 0; i < n; ++i) r += a[i];
    return r;
  }
  if (n <= 128) {
    double r[8];
    for (int j = 0; j < 8; ++j) r[j] = a[j];
    long i = 8;
    for (; i < n - (n % 8); i += 8)
      for (int j = 0; j < 8; ++j) r[j] += a[i + j];
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += a[i];
    return res;
  }
  long n2 = n / 2;
  n2 -= n2 % 8;
  return np_pairwise_sum(a, n2) + np_pairwise_sum(a + n2, n - n2);
}

extern "C" {

yms_status yms_map_match(int n_images, const float* det_boxes, const float* det_scores, const int* det_labels,
                         const int* det_off, const float* gt_boxes, const int* gt_labels, const int* gt_off,
                         uint8_t* tp, uint8_t* kept, int* rank_ws, int max_gt_per_image, void* stream) {
  if (n_images <= 0) return YMS_OK;
  if (!det_off || !gt_off || !tp || !kept || !rank_ws) return YMS_ERR_INVALID;
  if (max_gt_per_image > MAP_MAX_GT) return YMS_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(map_match_kernel, dim3((unsigned)n_images), dim3(64), 0, (hipStream_t)stream, det_boxes,
                     det_scores, det_labels, det_off, gt_boxes, gt_labels, gt_off, tp, kept, rank_ws);
  return launch_status();
}

// host: per-class precision / recall over the whole evaluation set (COCOeval.accumulate at one
// IoU threshold, area 'all', maxDets 100).  Inputs are host arrays in evaluation order.
yms_status yms_map_accumulate(int n_det, const float* scores, const int* labels, const int* image,
                              const uint8_t* tp, const uint8_t* kept, int n_classes, const int* n_gt,
                              double* ap, double* map) {
  if (n_det < 0 || n_classes <= 0 || !n_gt || !ap || !map) return YMS_ERR_INVALID;
  if (n_det > 0 && (!scores || !labels || !image || !tp || !kept)) return YMS_ERR_INVALID;
  std::vector<std::vector<int>> by(n_classes);
  for (int i = 0; i < n_det; ++i)
    if (kept[i] && labels[i] >= 0 && labels[i] < n_classes) by[labels[i]].push_back(i);
  const double eps = std::nextafter(1.0, 2.0) - 1.0;   // np.spacing(1)
  std::vector<double> aps;
  for (int c = 0; c < n_classes; ++c) {
    ap[c] = -1.0;
    if (n_gt[c] <= 0) continue;
    std::vector<int>& v = by[c];
    std::stable_sort(v.begin(), v.end(), [&](int a, int b) {
      if (scores[a] != scores[b]) return scores[a] > scores[b];
      if (image[a] != image[b]) return image[a] < image[b];
      return a < b;
    });
    const int nd = (int)v.size();
    std::vector<double> rc(nd), pr(nd);
    double tps = 0.0, fps = 0.0;
    for (int k = 0; k < nd; ++k) {
      if (tp[v[k]]) tps += 1.0; else fps += 1.0;
      rc[k] = tps / (double)n_gt[c];
      pr[k] = tps / (fps + tps + eps);
    }
    for (int k = nd - 1; k > 0; --k)
      if (pr[k] > pr[k - 1]) pr[k - 1] = pr[k];
    double q[101];
    for (int t = 0; t <= 100; ++t) {
      const double thr = (double)t * 0.01;      // np.linspace(0, 1, 101) = arange(101) * 0.01
      const int pi = (int)(std::lower_bound(rc.begin(), rc.end(), thr) - rc.begin());
      q[t] = pi < nd ? pr[pi] : 0.0;
    }
    ap[c] = np_pairwise_sum(q, 101) / 101.0;
    aps.push_back(ap[c]);
  }
  *map = aps.empty() ? -1.0 : np_pairwise_sum(aps.data(), (long)aps.size()) / (double)aps.size();
  return YMS_OK;
}

// T thresholds x 4 area ranges in one launch (COCOeval.evaluateImg on boxes; gt_crowd / gt_area: the
// annotations' iscrowd and area, each optional)
yms_status yms_map_match_coco_gt(int n_images, int n_det, const float* det_boxes, const float* det_scores,
                                 const int* det_labels, const int* det_off, const float* gt_boxes,
                                 const int* gt_labels, const int* gt_off, int n_thr, const double* iou_thrs,
                                 uint16_t* matched, uint16_t* ignored, uint8_t* gt_ignore, int* rank_ws,
                                 int max_gt_per_image, const uint8_t* gt_crowd, const float* gt_area, void* stream) {
  if (n_thr < 1 || n_thr > MAP_MAX_THR || !iou_thrs) return YMS_ERR_INVALID;
  MapCocoThr P;
  for (int t = 0; t < MAP_MAX_THR; ++t) P.thr[t] = t < n_thr ? iou_thrs[t] : 2.0;
  P.n = n_thr;
  for (int t = 0; t < n_thr; ++t)
    if (!(P.thr[t] > 0.0 && P.thr[t] <= 1.0) || (t > 0 && !(P.thr[t] > P.thr[t - 1]))) return YMS_ERR_INVALID;
  if (n_images <= 0) return YMS_OK;
  if (n_det < 0 || !det_off || !gt_off) return YMS_ERR_INVALID;
  if (n_det > 0 && (!det_boxes || !det_scores || !det_labels || !matched || !ignored || !rank_ws))
    return YMS_ERR_INVALID;
  if (max_gt_per_image < 0 || (max_gt_per_image > 0 && (!gt_boxes || !gt_labels || !gt_ignore))) return YMS_ERR_INVALID;
  if (max_gt_per_image > MAP_MAX_GT) return YMS_ERR_UNSUPPORTED;
  auto kernel = (gt_crowd || gt_area) ? map_match_coco_kernel<true> : map_match_coco_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)n_images), dim3(64 * MAP_COCO_WAVES), 0, (hipStream_t)stream, det_boxes,
                     det_scores, det_labels, det_off, gt_boxes, gt_labels, gt_crowd, gt_area, gt_off, P, (long)n_det,
                     matched, ignored, gt_ignore, rank_ws, rank_ws + n_det);
  return launch_status();
}

yms_status yms_map_match_coco(int n_images, int n_det, const float* det_boxes, const float* det_scores,
                              const int* det_labels, const int* det_off, const float* gt_boxes, const int* gt_labels,
                              const int* gt_off, int n_thr, const double* iou_thrs, uint16_t* matched,
                              uint16_t* ignored, uint8_t* gt_ignore, int* rank_ws, int max_gt_per_image,
                              void* stream) {
  return yms_map_match_coco_gt(n_images, n_det, det_boxes, det_scores, det_labels, det_off, gt_boxes, gt_labels,
                               gt_off, n_thr, iou_thrs, matched, ignored, gt_ignore, rank_ws, max_gt_per_image,
                               nullptr, nullptr, stream);
}

// the same matching on yms.ops.detect's padded layout, written into the epoch buffers of the device evaluator
yms_status yms_map_match_coco_fixed_gt(int n_images, int max_det, const float* det_boxes, const float* det_scores,
                                       const int* det_labels, const int* det_count, int max_gt, const float* gt_boxes,
                                       const int* gt_labels, const int* gt_count, int n_thr, const double* iou_thrs,
                                       int n_classes, long cap, long row0, float* score, int* label, int* rank,
                                       uint16_t* matched, uint16_t* ignored, int* npig, int* order_ws,
                                       const uint8_t* gt_crowd, const float* gt_area, void* stream) {
  if (n_thr < 1 || n_thr > MAP_MAX_THR || !iou_thrs) return YMS_ERR_INVALID;
  MapCocoThr P;
  for (int t = 0; t < MAP_MAX_THR; ++t) P.thr[t] = t < n_thr ? iou_thrs[t] : 2.0;
  P.n = n_thr;
  for (int t = 0; t < n_thr; ++t)
    if (!(P.thr[t] > 0.0 && P.thr[t] <= 1.0) || (t > 0 && !(P.thr[t] > P.thr[t - 1]))) return YMS_ERR_INVALID;
  if (max_det < 1 || max_det > MAP_FIXED_MAX_DET || n_classes < 1 || n_classes > MAP_MAX_CLASSES || max_gt < 0)
    return YMS_ERR_INVALID;
  if (max_gt > MAP_MAX_GT) return YMS_ERR_UNSUPPORTED;
  if (n_images <= 0) return YMS_OK;
  if (row0 < 0 || cap < 0 || row0 + (long)n_images * max_det > cap) return YMS_ERR_INVALID;
  if (!det_boxes || !det_scores || !det_labels || !det_count || !gt_count || !score || !label || !rank || !matched ||
      !ignored || !npig || !order_ws)
    return YMS_ERR_INVALID;
  if (max_gt > 0 && (!gt_boxes || !gt_labels)) return YMS_ERR_INVALID;
  auto kernel = (gt_crowd || gt_area) ? map_match_coco_fixed_kernel<true> : map_match_coco_fixed_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)n_images), dim3(64 * MAP_COCO_WAVES), 0, (hipStream_t)stream, det_boxes,
                     det_scores, det_labels, det_count, max_det, gt_boxes, gt_labels, gt_crowd, gt_area, gt_count,
                     max_gt, P, n_classes, cap, row0, score, label, rank, matched, ignored, npig, order_ws);
  return launch_status();
}

yms_status yms_map_match_coco_fixed(int n_images, int max_det, const float* det_boxes, const float* det_scores,
                                    const int* det_labels, const int* det_count, int max_gt, const float* gt_boxes,
                                    const int* gt_labels, const int* gt_count, int n_thr, const double* iou_thrs,
                                    int n_classes, long cap, long row0, float* score, int* label, int* rank,
                                    uint16_t* matched, uint16_t* ignored, int* npig, int* order_ws, void* stream) {
  return yms_map_match_coco_fixed_gt(n_images, max_det, det_boxes, det_scores, det_labels, det_count, max_gt,
                                     gt_boxes, gt_labels, gt_count, n_thr, iou_thrs, n_classes, cap, row0, score,
                                     label, rank, matched, ignored, npig, order_ws, nullptr, nullptr, stream);
}

// host: COCOeval.accumulate over T thresholds, 4 area ranges and maxDets 1 / 10 / 100
yms_status yms_map_accumulate_coco(int n_det, const float* scores, const int* labels, const int* image,
                                   const int* rank, const uint16_t* matched, const uint16_t* ignored, int n_thr,
                                   int n_classes, const int* npig, double* precision, double* recall) {
  if (n_det < 0 || n_classes <= 0 || n_thr < 1 || n_thr > MAP_MAX_THR || !npig || !precision || !recall)
    return YMS_ERR_INVALID;
  if (n_det > 0 && (!scores || !labels || !image || !rank || !matched || !ignored)) return YMS_ERR_INVALID;
  constexpr int NA = MAP_N_AREA, NM = 3, NR = 101;
  const int max_dets[NM] = {1, 10, MAP_MAXDET};
  const long K = n_classes;
  std::fill(precision, precision + (long)n_thr * NR * K * NA * NM, -1.0);
  std::fill(recall, recall + (long)n_thr * K * NA * NM, -1.0);
  std::vector<std::vector<int>> by(n_classes);
  for (int i = 0; i < n_det; ++i)
    if (rank[i] >= 0 && rank[i] < MAP_MAXDET && labels[i] >= 0 && labels[i] < n_classes) by[labels[i]].push_back(i);
  const double eps = std::nextafter(1.0, 2.0) - 1.0;   // np.spacing(1)
  std::vector<int> sel;
  std::vector<double> rc, pr;
  for (int c = 0; c < n_classes; ++c) {
    std::vector<int>& v = by[c];
    std::stable_sort(v.begin(), v.end(), [&](int x, int y) {
      if (scores[x] != scores[y]) return scores[x] > scores[y];
      if (image[x] != image[y]) return image[x] < image[y];
      return x < y;
    });
    for (int a = 0; a < NA; ++a) {
      const int np_ = npig[c * NA + a];
      if (np_ <= 0) continue;
      for (int mi = 0; mi < NM; ++mi) {
        sel.clear();
        for (int i : v)
          if (rank[i] < max_dets[mi]) sel.push_back(i);
        const int nd = (int)sel.size();
        rc.resize(nd);
        pr.resize(nd);
        for (int t = 0; t < n_thr; ++t) {
          double tps = 0.0, fps = 0.0;
          for (int k = 0; k < nd; ++k) {
            const long i = (long)a * n_det + sel[k];
            const bool m = (matched[i] >> t) & 1, ig = (ignored[i] >> t) & 1;
            if (!ig) { if (m) tps += 1.0; else fps += 1.0; }
            rc[k] = tps / (double)np_;
            pr[k] = tps / (fps + tps + eps);
          }
          for (int k = nd - 1; k > 0; --k)
            if (pr[k] > pr[k - 1]) pr[k - 1] = pr[k];
          recall[(((long)t * K + c) * NA + a) * NM + mi] = nd ? rc[nd - 1] : 0.0;
          for (int r = 0; r < NR; ++r) {
            const double thr = (double)r * 0.01;      // np.linspace(0, 1, 101) = arange(101) * 0.01
            const int pi = (int)(std::lower_bound(rc.begin(), rc.end(), thr) - rc.begin());
            precision[((((long)t * NR + r) * K + c) * NA + a) * NM + mi] = pi < nd ? pr[pi] : 0.0;
          }
        }
      }
    }
  }
  return YMS_OK;
}

}  // extern "C"
