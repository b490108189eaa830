// Optimizer step for the flat-arena training loop: SGD / Adam / AdamW, weight EMA (two rules), gradient-norm
// clipping, the device-side non-finite skip and a piecewise schedule of the learning rate and momentum
// evaluated on the device, in a launch count that does not depend on the number of tensors.
//
// The tensors are rows of a device table (yms_optim_chunk, include/yms.h): every row is at most CHUNK
// consecutive elements of ONE tensor and one block takes one row, so a block's work is the same
// whichever tensor it lands in.  Gradients are addressed as byte offsets from a per-call base (the
// backward's flat arena), so one table serves every arena and a captured graph.
//
// Streaming kernels: 20 B (SGD) / 28 B (Adam) per element, + 8 B with the EMA.  A full row whose
// parameter / state / EMA addresses are 16-B aligned moves as four float4 per thread and stream, all
// issued before the block's scalar prologue (norm re-reduction, fp64 bias corrections) so the
// prologue's latency hides under the loads; the gradient, a view at an arbitrary element offset of
// the arena, is read as float4 when its address allows and as four dwords otherwise (the wave still
// covers whole cache lines).  Short rows and unaligned tensors take the element-wise path.
#include <math.h>

#include "yms_common.hpp"

namespace yms {
namespace {

constexpr int OPT_CHUNK = 4096;                    // elements per table row
constexpr int OPT_BLOCK = 256;
constexpr int OPT_V4 = OPT_CHUNK / OPT_BLOCK / 4;  // float4 per thread and stream of a full row
constexpr int OPT_MAX_PARTIALS = OPT_BLOCK * 128;  // the re-reduction's per-thread chain stays <= 128

__device__ __forceinline__ bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

__device__ __forceinline__ const float* grad_ptr(const yms_optim_chunk& c, const char* gbase) {
  return (c.flags & YMS_OPTIM_GRAD_ABS) ? reinterpret_cast<const float*>(static_cast<uintptr_t>(c.g))
                                        : reinterpret_cast<const float*>(gbase + c.g);
}

// Sum over the block in one fixed tree (xor butterflies, then the four waves in order): every lane
// of every block gets the same bits for the same inputs.
template <typename T>
__device__ __forceinline__ T block_sum(T v, T* red) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  const int w = threadIdx.x >> 6;
  lds_barrier();                 // red may still be read from an earlier call
  if ((threadIdx.x & 63) == 0) red[w] = v;
  lds_barrier();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// The gradient norm from yms_optim_grad_norm's partial sums: thread t adds partials t, t + 256, ...
// (<= 128 of them) and the block tree above finishes, in fp64, so every block of the update and the
// tick arrive at the same norm.
__device__ __forceinline__ float norm_from_partials(const float* partials, int np, double* red) {
  double a = 0.0;
  for (int i = threadIdx.x; i < np; i += OPT_BLOCK) a += (double)partials[i];
  return (float)sqrt(block_sum(a, red));
}

struct StepCoef {
  float clip;          // gradient scale (1 without clipping)
  float wd;            // AdamW: the decay factor 1 - lr wd
  float a, oma;        // SGD: momentum, -        Adam: beta1, 1 - beta1
  float b, omb;        // SGD: lr, -              Adam: beta2, 1 - beta2
  float step, bc2s;    // Adam: lr / bc1, sqrt(bc2)
  float eps;
  float ed, eomd;      // EMA: delta, 1 - delta
  int first, nesterov;
};

// The schedule (include/yms.h): the products of the factors that the segments holding group g
// contribute at index n, for the learning rate and for the momentum.  One lane, fp64.
__device__ __forceinline__ void sched_factors(const yms_optim_ext* ext, int g, double n, double& flr, double& fmom) {
  flr = 1.0;
  fmom = 1.0;
  const double ns = ext->nsegments;
  const int nseg = ns >= (double)YMS_OPTIM_MAX_SEGMENTS ? YMS_OPTIM_MAX_SEGMENTS : (ns >= 1.0 ? (int)ns : 0);   // nan: 0
  for (int s = 0; s < nseg; ++s) {
    const yms_optim_segment sg = ext->seg[s];
    const bool lr = sg.target == YMS_OPTIM_SCHED_LR;
    if (!(sg.end > sg.begin) || !((sg.groups >> g) & 1) || (!lr && sg.target != YMS_OPTIM_SCHED_MOMENTUM) ||
        (sg.shape != YMS_OPTIM_SCHED_LINEAR && sg.shape != YMS_OPTIM_SCHED_COSINE))
      continue;
    double f;
    if (n <= sg.begin) {
      f = sg.from;
    } else if (n >= sg.end) {
      f = sg.to;
    } else {
      const double u = (n - sg.begin) / (sg.end - sg.begin);
      f = sg.shape == YMS_OPTIM_SCHED_LINEAR ? sg.from + (sg.to - sg.from) * u
                                             : sg.to + (sg.from - sg.to) * (1.0 + cospi(u)) / 2.0;
      // (cospi, not cos(pi u): no large-argument reduction, which cost Adam's update a wave per SIMD)
    }
    if (lr) flr *= f; else fmom *= f;
  }
}

template <int KIND>
__device__ __forceinline__ void update1(const StepCoef& k, float g, float& p, float& s0, float& s1) {
  float d;
  if (KIND == YMS_OPTIM_ADAMW) {
    p = p * k.wd;
    d = g * k.clip;
  } else {
    d = g * k.clip + k.wd * p;
  }
  if (KIND == YMS_OPTIM_SGD) {
    const float b = k.first ? d : k.a * s0 + d;
    s0 = b;
    p = p - k.b * (k.nesterov ? d + k.a * b : b);
  } else {
    const float m = k.a * s0 + k.oma * d;
    const float v = k.b * s1 + k.omb * (d * d);
    s0 = m;
    s1 = v;
    const float den = sqrtf(v) / k.bc2s + k.eps;
    p = p - k.step * (m / den);
  }
}

// EXT: an extension record is given.  Without one the kernel is the code it was before the record
// existed (the schedule and the second EMA rule are compiled out), so yms_optim_step's cost is too.
template <int KIND, bool EXT>
__global__ __launch_bounds__(OPT_BLOCK) void optim_step_kernel(const yms_optim_chunk* __restrict__ table,
                                                                const char* gbase, const yms_optim_hyper* hy,
                                                                const yms_optim_ext* ext, const yms_optim_counters* cnt,
                                                                const float* partials, int np) {
  __shared__ double red[4];
  __shared__ StepCoef shk;
  const yms_optim_chunk c = table[blockIdx.x];
  const int tid = threadIdx.x;
  const bool upd = !(c.flags & YMS_OPTIM_GRAD_NONE) && c.s0 && (KIND == YMS_OPTIM_SGD || c.s1);
  const bool ema = (c.flags & YMS_OPTIM_EMA) && c.e;
  if (!upd && !ema) return;
  const float* g = upd ? grad_ptr(c, gbase) : nullptr;
  float* s1 = KIND != YMS_OPTIM_SGD ? c.s1 : nullptr;

  // a full row with aligned tensors: every load goes out before the prologue
  const bool wide = c.n == OPT_CHUNK && al16(c.p) && (!upd || (al16(c.s0) && al16(s1))) && (!ema || al16(c.e));
  const bool gwide = upd && al16(g);
  f32x4 P[OPT_V4], G[OPT_V4], S0[OPT_V4], S1[OPT_V4], E[OPT_V4];
  if (wide) {
#pragma unroll
    for (int j = 0; j < OPT_V4; ++j) {
      const int i = j * (OPT_BLOCK * 4) + tid * 4;
      P[j] = *reinterpret_cast<const f32x4*>(c.p + i);
      if (upd) {
        if (gwide) {
          G[j] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(g + i));
        } else {
#pragma unroll
          for (int q = 0; q < 4; ++q) G[j][q] = g[i + q];
        }
        S0[j] = *reinterpret_cast<const f32x4*>(c.s0 + i);
        if (KIND != YMS_OPTIM_SGD) S1[j] = *reinterpret_cast<const f32x4*>(s1 + i);
      }
      if (ema) E[j] = *reinterpret_cast<const f32x4*>(c.e + i);
    }
  }

  float norm = 0.0f;
  if (partials) {
    norm = norm_from_partials(partials, np, red);
    if (!(fabsf(norm) <= 3.402823466e38f) && hy->skip_nonfinite != 0.0) return;   // inf or nan: write nothing
  }
  if (tid == 0) {
    StepCoef k;
    const double* h = hy->group[c.group];
    double lr = h[0], b1 = h[1];
    const double b2 = h[2];
    if (EXT) {
      double flr, fmom;
      sched_factors(ext, c.group, (double)cnt->step + (double)cnt->skipped, flr, fmom);
      lr *= flr;
      b1 *= fmom;
    }
    k.clip = 1.0f;
    if (partials && hy->max_norm > 0.0) {
      const float c0 = (float)hy->max_norm / (norm + 1e-6f);
      k.clip = c0 > 1.0f ? 1.0f : c0;        // a nan norm passes through, as torch.clamp does
    }
    k.wd = KIND == YMS_OPTIM_ADAMW ? (float)(1.0 - lr * h[4]) : (float)h[4];
    k.eps = (float)h[3];
    k.nesterov = h[5] != 0.0;
    k.first = cnt->step == 0;
    if (KIND == YMS_OPTIM_SGD) {
      k.a = (float)b1; k.oma = 0.0f; k.b = (float)lr; k.omb = 0.0f; k.step = 0.0f; k.bc2s = 1.0f;
    } else {
      const double t = (double)cnt->step + 1.0;
      const double bc1 = 1.0 - pow(b1, t), bc2 = 1.0 - pow(b2, t);
      k.a = (float)b1; k.oma = (float)(1.0 - b1); k.b = (float)b2; k.omb = (float)(1.0 - b2);
      k.step = (float)(lr / bc1);
      k.bc2s = (float)sqrt(bc2);
    }
    double dl = hy->ema_decay;
    if (EXT && ext->ema_rule == (double)YMS_OPTIM_EMA_EXPMOM) {
      // dl is the momentum floor m here; the EMA keeps 1 - mu of itself
      if (hy->ema_tau > 0.0) dl += (1.0 - dl) * exp(-((double)cnt->ema_step + 1.0) / hy->ema_tau);
      k.ed = (float)(1.0 - dl);
      k.eomd = (float)dl;
    } else {
      if (hy->ema_tau > 0.0) dl *= 1.0 - exp(-((double)cnt->ema_step + 1.0) / hy->ema_tau);
      k.ed = (float)dl;
      k.eomd = (float)(1.0 - dl);
    }
    shk = k;
  }
  lds_barrier();
  const StepCoef k = shk;

  if (wide) {
#pragma unroll
    for (int j = 0; j < OPT_V4; ++j) {
      const int i = j * (OPT_BLOCK * 4) + tid * 4;
      if (upd) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          float p = P[j][q], a = S0[j][q], b = KIND != YMS_OPTIM_SGD ? S1[j][q] : 0.0f;
          update1<KIND>(k, G[j][q], p, a, b);
          P[j][q] = p; S0[j][q] = a; S1[j][q] = b;
        }
        *reinterpret_cast<f32x4*>(c.p + i) = P[j];
        *reinterpret_cast<f32x4*>(c.s0 + i) = S0[j];
        if (KIND != YMS_OPTIM_SGD) *reinterpret_cast<f32x4*>(s1 + i) = S1[j];
      }
      if (ema) {
#pragma unroll
        for (int q = 0; q < 4; ++q) E[j][q] = k.ed * E[j][q] + k.eomd * P[j][q];
        *reinterpret_cast<f32x4*>(c.e + i) = E[j];
      }
    }
    return;
  }
#pragma unroll 4
  for (int i = tid; i < c.n; i += OPT_BLOCK) {
    float p = c.p[i];
    if (upd) {
      float a = c.s0[i], b = KIND != YMS_OPTIM_SGD ? s1[i] : 0.0f;
      update1<KIND>(k, g[i], p, a, b);
      c.p[i] = p;
      c.s0[i] = a;
      if (KIND != YMS_OPTIM_SGD) s1[i] = b;
    }
    if (ema) c.e[i] = k.ed * c.e[i] + k.eomd * p;
  }
}

// After the update (stream order): advance the counters.  One block; lane 0 writes.
// With sched_out, lanes 0 .. 15 first store the learning rate and momentum this call ran at, one
// (group, target) each, from the counters as the update read them.
__global__ __launch_bounds__(OPT_BLOCK) void optim_tick_kernel(const yms_optim_hyper* hy, const yms_optim_ext* ext,
                                                                yms_optim_counters* cnt, double* sched_out,
                                                                const float* partials, int np) {
  __shared__ double red[4];
  const int step0 = cnt->step, skipped0 = cnt->skipped;
  if (sched_out && threadIdx.x < 2 * YMS_OPTIM_MAX_GROUPS) {
    const int g = threadIdx.x >> 1, which = threadIdx.x & 1;
    double f[2] = {1.0, 1.0};
    if (ext) sched_factors(ext, g, (double)step0 + (double)skipped0, f[0], f[1]);
    sched_out[threadIdx.x] = hy->group[g][which] * (which ? f[1] : f[0]);
  }
  float norm = 0.0f;
  bool skip = false;
  if (partials) {
    norm = norm_from_partials(partials, np, red);
    skip = !(fabsf(norm) <= 3.402823466e38f) && hy->skip_nonfinite != 0.0;
  }
  if (threadIdx.x == 0) {
    if (skip) {
      cnt->skipped = skipped0 + 1;
    } else {
      cnt->step = step0 + 1;
      cnt->ema_step = cnt->ema_step + 1;
    }
    if (partials) cnt->grad_norm = norm;
  }
}

// Sum of squares of the rows b, b + gridDim.x, ... of the table -> partials[b].  Per thread: a fixed
// tree over its <= 16 elements of a row, then one addition per row (<= 128 rows per block).
__global__ __launch_bounds__(OPT_BLOCK) void optim_norm_kernel(const yms_optim_chunk* __restrict__ table, long nchunks,
                                                                const char* gbase, float* partials) {
  __shared__ float red[4];
  const int tid = threadIdx.x;
  float acc = 0.0f;
  for (long r = blockIdx.x; r < nchunks; r += gridDim.x) {
    const yms_optim_chunk c = table[r];
    if ((c.flags & YMS_OPTIM_GRAD_NONE) || !c.s0) continue;
    const float* g = grad_ptr(c, gbase);
    float s = 0.0f;
    if (c.n == OPT_CHUNK) {
      // the same tree whether the arena offset allows float4 reads or not: the norm does not
      // depend on where the arena puts a tensor
      const bool gwide = al16(g);
      float q[OPT_V4];
#pragma unroll
      for (int j = 0; j < OPT_V4; ++j) {
        const int i = j * (OPT_BLOCK * 4) + tid * 4;
        f32x4 v;
        if (gwide) {
          v = *reinterpret_cast<const f32x4*>(g + i);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = g[i + e];
        }
        q[j] = (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
      }
      s = (q[0] + q[1]) + (q[2] + q[3]);
    } else {
#pragma unroll 4
      for (int i = tid; i < c.n; i += OPT_BLOCK) s += g[i] * g[i];
    }
    acc += s;
  }
  const float tot = block_sum(acc, red);
  if (tid == 0) partials[blockIdx.x] = tot;
}

__global__ __launch_bounds__(OPT_BLOCK) void optim_swap_kernel(const yms_optim_chunk* __restrict__ table) {
  const yms_optim_chunk c = table[blockIdx.x];
  if (!(c.flags & YMS_OPTIM_EMA) || !c.e) return;
  const int tid = threadIdx.x;
  if (c.n == OPT_CHUNK && al16(c.p) && al16(c.e)) {
    f32x4 P[OPT_V4], E[OPT_V4];
#pragma unroll
    for (int j = 0; j < OPT_V4; ++j) {
      const int i = j * (OPT_BLOCK * 4) + tid * 4;
      P[j] = *reinterpret_cast<const f32x4*>(c.p + i);
      E[j] = *reinterpret_cast<const f32x4*>(c.e + i);
    }
#pragma unroll
    for (int j = 0; j < OPT_V4; ++j) {
      const int i = j * (OPT_BLOCK * 4) + tid * 4;
      *reinterpret_cast<f32x4*>(c.p + i) = E[j];
      *reinterpret_cast<f32x4*>(c.e + i) = P[j];
    }
    return;
  }
  for (int i = tid; i < c.n; i += OPT_BLOCK) {
    const float p = c.p[i], e = c.e[i];
    c.p[i] = e;
    c.e[i] = p;
  }
}

// Host: a job is usable when its fields are consistent on their own and with the buffers given.
bool job_ok(const yms_optim_job& j) {
  const int known = YMS_OPTIM_GRAD_NONE | YMS_OPTIM_GRAD_ABS | YMS_OPTIM_EMA;
  if (!j.param || j.count < 1 || j.group < 0 || j.group >= YMS_OPTIM_MAX_GROUPS || (j.flags & ~known)) return false;
  if ((j.flags & YMS_OPTIM_GRAD_NONE) && (j.flags & YMS_OPTIM_GRAD_ABS)) return false;
  if (!(j.flags & YMS_OPTIM_GRAD_NONE)) {
    if (j.grad < 0 || (j.grad & 3) || j.state0 < 0) return false;
    if ((j.flags & YMS_OPTIM_GRAD_ABS) && j.grad == 0) return false;
  }
  if (j.state0 < -1 || j.state1 < -1 || j.ema < -1) return false;
  if ((j.flags & YMS_OPTIM_EMA) && j.ema < 0) return false;
  return true;
}

long table_chunks(int njobs, const yms_optim_job* jobs) {
  if (njobs < 0 || (njobs > 0 && !jobs)) return -1;
  long n = 0;
  for (int i = 0; i < njobs; ++i) {
    if (!job_ok(jobs[i])) return -1;
    n += (long)((jobs[i].count + OPT_CHUNK - 1) / OPT_CHUNK);
  }
  return n;
}

template <int KIND>
void launch_step(bool ext, unsigned grid, hipStream_t st, const yms_optim_chunk* t, const char* gb,
                 const yms_optim_hyper* hy, const yms_optim_ext* ex, const yms_optim_counters* cnt, const float* partials,
                 int np) {
  if (ext)
    hipLaunchKernelGGL((optim_step_kernel<KIND, true>), dim3(grid), dim3(OPT_BLOCK), 0, st, t, gb, hy, ex, cnt, partials,
                       np);
  else
    hipLaunchKernelGGL((optim_step_kernel<KIND, false>), dim3(grid), dim3(OPT_BLOCK), 0, st, t, gb, hy, ex, cnt,
                       partials, np);
}

}  // namespace
}  // namespace yms

using namespace yms;

extern "C" {

int yms_optim_chunk_elems(void) { return OPT_CHUNK; }

long yms_optim_table_chunks(int njobs, const yms_optim_job* jobs) { return table_chunks(njobs, jobs); }

size_t yms_optim_table_bytes(int njobs, const yms_optim_job* jobs) {
  const long n = table_chunks(njobs, jobs);
  return n < 0 ? 0 : (size_t)n * sizeof(yms_optim_chunk);
}

yms_status yms_optim_table_build(int njobs, const yms_optim_job* jobs, float* state0, float* state1, float* ema,
                                 void* table, size_t table_bytes) {
  const long n = table_chunks(njobs, jobs);
  if (n < 0 || !table || table_bytes < (size_t)n * sizeof(yms_optim_chunk)) return YMS_ERR_INVALID;
  for (int i = 0; i < njobs; ++i) {
    const yms_optim_job& j = jobs[i];
    if ((j.state0 >= 0 && !state0) || (j.state1 >= 0 && !state1) || (j.ema >= 0 && !ema)) return YMS_ERR_INVALID;
  }
  yms_optim_chunk* out = static_cast<yms_optim_chunk*>(table);
  for (int i = 0; i < njobs; ++i) {
    const yms_optim_job& j = jobs[i];
    for (int64_t o = 0; o < j.count; o += OPT_CHUNK) {
      yms_optim_chunk c;
      c.p = static_cast<float*>(j.param) + o;
      c.g = (j.flags & YMS_OPTIM_GRAD_NONE) ? 0 : j.grad + 4 * o;
      c.s0 = j.state0 >= 0 ? state0 + j.state0 + o : nullptr;
      c.s1 = j.state1 >= 0 ? state1 + j.state1 + o : nullptr;
      c.e = j.ema >= 0 ? ema + j.ema + o : nullptr;
      c.n = (int)(j.count - o < OPT_CHUNK ? j.count - o : OPT_CHUNK);
      c.group = (short)j.group;
      c.flags = (short)j.flags;
      *out++ = c;
    }
  }
  return YMS_OK;
}

int yms_optim_norm_partials(long nchunks) {
  if (nchunks <= 0) return 0;
  const long per128 = (nchunks + 127) / 128;
  const long g = nchunks < 1024 ? nchunks : (per128 > 1024 ? per128 : 1024);
  return g > OPT_MAX_PARTIALS ? -1 : (int)g;
}

yms_status yms_optim_grad_norm(const void* table, long nchunks, const void* grad_base, float* partials,
                               void* stream) {
  if (!table || nchunks <= 0 || !partials) return YMS_ERR_INVALID;
  const int g = yms_optim_norm_partials(nchunks);
  if (g < 0) return YMS_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(optim_norm_kernel, dim3((unsigned)g), dim3(OPT_BLOCK), 0, (hipStream_t)stream,
                     static_cast<const yms_optim_chunk*>(table), nchunks, static_cast<const char*>(grad_base),
                     partials);
  return launch_status();
}

yms_status yms_optim_step_ext(int kind, const void* table, long nchunks, const void* grad_base,
                              const yms_optim_hyper* hyper, const yms_optim_ext* ext, yms_optim_counters* counters,
                              double* sched_out, const float* partials, int npartials, void* stream) {
  if ((kind != YMS_OPTIM_SGD && kind != YMS_OPTIM_ADAM && kind != YMS_OPTIM_ADAMW) || !table || nchunks <= 0 ||
      nchunks > 0x7fffffffL || !hyper || !counters || npartials < 0 || (partials != nullptr) != (npartials > 0))
    return YMS_ERR_INVALID;
  if (npartials > OPT_MAX_PARTIALS) return YMS_ERR_UNSUPPORTED;
  const yms_optim_chunk* t = static_cast<const yms_optim_chunk*>(table);
  const char* gb = static_cast<const char*>(grad_base);
  hipStream_t st = (hipStream_t)stream;
  const unsigned grid = (unsigned)nchunks;
  if (kind == YMS_OPTIM_SGD)
    launch_step<YMS_OPTIM_SGD>(ext != nullptr, grid, st, t, gb, hyper, ext, counters, partials, npartials);
  else if (kind == YMS_OPTIM_ADAM)
    launch_step<YMS_OPTIM_ADAM>(ext != nullptr, grid, st, t, gb, hyper, ext, counters, partials, npartials);
  else
    launch_step<YMS_OPTIM_ADAMW>(ext != nullptr, grid, st, t, gb, hyper, ext, counters, partials, npartials);
  hipLaunchKernelGGL(optim_tick_kernel, dim3(1), dim3(OPT_BLOCK), 0, st, hyper, ext, counters, sched_out, partials,
                     npartials);
  return launch_status();
}

yms_status yms_optim_step(int kind, const void* table, long nchunks, const void* grad_base,
                          const yms_optim_hyper* hyper, yms_optim_counters* counters, const float* partials,
                          int npartials, void* stream) {
  if (kind != YMS_OPTIM_SGD && kind != YMS_OPTIM_ADAM) return YMS_ERR_INVALID;
  return yms_optim_step_ext(kind, table, nchunks, grad_base, hyper, nullptr, counters, nullptr, partials, npartials,
                            stream);
}

yms_status yms_optim_swap(const void* table, long nchunks, void* stream) {
  if (!table || nchunks <= 0 || nchunks > 0x7fffffffL) return YMS_ERR_INVALID;
  hipLaunchKernelGGL(optim_swap_kernel, dim3((unsigned)nchunks), dim3(OPT_BLOCK), 0, (hipStream_t)stream,
                     static_cast<const yms_optim_chunk*>(table));
  return launch_status();
}

}  // extern "C"
