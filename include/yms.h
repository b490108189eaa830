/* yms.h -- C-ABI of the MI355X-native YOLO-MS / YOLOv8 detector hot path.
 *
 * Plain C, no torch types: raw device pointers, sizes and a hipStream_t passed as void*.
 * Every call is stream-ordered and asynchronous, allocates nothing (caller-owned outputs
 * and workspaces), is thread-compatible, and returns a status instead of throwing.
 *
 * Activation layout: NHWC.  A "view" of an activation is (ptr, ld, off): element
 * (n, y, x, c) lives at ptr[((n*H + y)*W + x)*ld + off + c].  ld and off are multiples of 8
 * elements; channels in [C, round_up(C,8)) of a buffer are kept zero by the producers.
 * dtype: YMS_F32 / YMS_BF16 / YMS_F16 for activations and packed weights; every
 * accumulation, BN statistic and parameter gradient is fp32.
 *
 * Reference interfaces each entry point replaces (paths relative to the reference repo
 * rafaelghiorzi/YOLO-MS):
 *   yms_conv_fwd            components.py:69-77 Conv.forward (Conv2d->BN->SiLU), the
 *                           Bottleneck residual add (:87-93), the C2f/SPPF/neck/head torch.cat
 *                           (:119, :146, yolov8_neck.py:79-91, yolov8_head.py:122) via y_off,
 *                           and the head's biased 1x1 nn.Conv2d (yolov8_head.py:86-109)
 *   yms_conv_dgrad/_wgrad   autograd of the above (train.py:371 loss.backward())
 *   yms_bn_*                components.py:73 nn.BatchNorm2d(eps=1e-3, momentum=0.03), train+eval
 *   yms_sppf_pool_*         components.py:136-146 three chained MaxPool2d(5,1,2)
 *   yms_upsample2x_*        components.py:153-160 Upsample (nearest x2)
 *   yms_head_decode         yolov8_head.py:127-158 make_anchors + DFL (components.py:162-191)
 *   yms_nms_*               train.py:63-113 / tools/test.py:166-218 post-process and the
 *                           torchvision.ops.nms(boxes, scores, iou) call at train.py:93
 *   yms_det_*               nothing in the reference: the COCO evaluation protocol (multi-label
 *                           candidates, max_nms / max_det caps, letterbox unmap) around
 *                           yms_nms_classwise, opt-in
 *   yms_tta_merge,          nothing in the reference: test-time augmentation's view merge and box
 *   yms_det_finalize_vote   voting around the same detect, opt-in
 *   yms_tile_merge          nothing in the reference: tiled (sliced) inference of large images, the
 *                           gather of every tile's predictions in front of the same detect, opt-in
 *   yms_resize_normalize,   tools/dataset.py:84-134 transform list + collate_fn's stack (:260)
 *   yms_augment_normalize
 *   yms_mosaic_normalize    the config's `mosaic` / `mixup` keys, which dataset.py never reads:
 *                           YOLOv5 load_mosaic / random_perspective / mixup semantics, opt-in
 *   yms_box_targets         the boxes of those samples (dataset.py:84-88, :218-228 filters) from a device
 *                           annotation table, for the device-resident loader (yms.cache), opt-in
 *   yms_optim_*             tools/utils.py:11-25 get_optimizer's torch.optim.SGD / Adam step, plus the
 *                           weight EMA, clip_grad_norm_ and non-finite guard (train.py:365,376), opt-in
 */
#ifndef YMS_H
#define YMS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int yms_status;
#define YMS_OK 0
#define YMS_ERR_INVALID 1
#define YMS_ERR_UNSUPPORTED 2
#define YMS_ERR_LAUNCH 3

#define YMS_F32 0
#define YMS_BF16 1
#define YMS_F16 2

#define YMS_ACT_NONE 0
#define YMS_ACT_SILU 1

/* One convolution: input [n, h, w, cin] -> output [n, ho, wo, cout], square kernel k,
 * stride, pad (ho = (h + 2*pad - k)/stride + 1). */
typedef struct {
  int n, h, w, cin, cout, k, stride, pad, ho, wo, dtype;
} yms_conv_shape;

const char* yms_version(void);
/* A new stream restricted to ncus CUs (mode 0: lowest CU indices, 1: spread), for the backward's
 * weight-gradient side stream (hipExtStreamCreateWithCUMask).  *stream_out: hipStream_t. */
yms_status yms_stream_create_cu_subset(int ncus, int mode, void** stream_out);
const char* yms_status_string(yms_status s);

/* ---- weights ------------------------------------------------------------------------ */
/* Elements of the packed weight for the forward / dgrad GEMM (16-bit or fp32 per dtype). */
size_t yms_conv_packed_elems(const yms_conv_shape* s, int for_dgrad);
/* w: fp32 [cout][cin][k][k] (nn.Conv2d layout) -> packed dtype layout.
 * for_dgrad = 0: [cout_pad][K] with K = (kh, kw, cin_pad8) chunk order;
 * for_dgrad = 1: [cin_pad][K'] with K' = (kh, kw, cout_pad8). */
yms_status yms_conv_pack_weight(const yms_conv_shape* s, const float* w, void* packed,
                                int for_dgrad, void* stream);

/* Batched packing (one launch for all of a plan's packs; training repacks every step).
 * yms_pack_job_init fills a job on the host (YMS_ERR_UNSUPPORTED for stride-2 dgrad packs,
 * which keep yms_conv_pack_weight); the job array must be in device memory for the launch.
 * Each job's `packed` is taken as a byte offset from dst_base (dst_base NULL: absolute), so one
 * device job table serves every arena (and HIP-graph capture needs no host->device copy). */
typedef struct {
  const float* w;
  void* packed;
  int cout, cin, ks, rows, kp_elems, c8_in, for_dgrad, dtype;
  /* optional second source (sibling convs packed as one, yms_pack_job_init sets NULL / 0): output
   * channels co >= split read w2[co - split] instead of w[co] */
  const float* w2;
  int split;
} yms_pack_job;
yms_status yms_pack_job_init(const yms_conv_shape* s, const float* w, void* packed, int for_dgrad,
                             yms_pack_job* job);
yms_status yms_conv_pack_weights_batched(int njobs, const yms_pack_job* jobs_dev, void* dst_base, void* stream);

/* ---- convolution (implicit GEMM on MFMA) --------------------------------------------- */
/* Rows of BN partial statistics written by yms_conv_fwd(stats != NULL): fp32 -- one per 128
 * output pixels; bf16/f16 -- one per persistent block (and 128-row half of its tiles).  The stats
 * workspace is [rows][2][stats_ld] floats followed by [rows] float pixel counts (so
 * rows * (2*stats_ld + 1) floats), stats_ld = yms_conv_stats_ld(). */
int yms_conv_stats_rows(const yms_conv_shape* s);
int yms_conv_stats_ld(const yms_conv_shape* s);
/* Process-wide route switch of the direct small-channel 3x3 kernel (conv_direct.hip; default on,
 * YMS_DIRECT=0 in the environment at the first call turns it off).  on = 0 / 1 sets it, on < 0 only
 * queries; returns the previous setting.  It changes yms_conv_stats_rows, so callers flip it only
 * while no plan sized under the other setting is in use (tests and A/B runs). */
int yms_conv_direct_set(int on);
/* Process-wide CU count that sizes the persistent grids, strip lengths, units per block and split-K
 * counts of the conv, depthwise and weight-gradient kernels.  n > 0: that count from now on; n == 0:
 * back to the device's; n < 0: query only.  Returns the previous setting (0 = the device's).  It
 * changes yms_conv_stats_rows, yms_conv_dgrad_bnred_rows and the *_wgrad_ws_bytes queries, so callers
 * flip it only while no plan sized under another setting is in use (tests and A/B runs). */
int yms_cu_count_set(int n);
/* Forward.  stats == NULL: y = act(conv(x)*scale[c] + shift[c]) (+ res) (scale/shift may
 * be NULL = identity).  stats != NULL (training): y = conv(x) (pre-BN z) and statistics rows
 * (sum z, sum (z - row mean)^2, pixel count) into stats. */
yms_status yms_conv_fwd(const yms_conv_shape* s, const void* x, int x_ld, int x_off,
                        const void* wpacked, void* y, int y_ld, int y_off,
                        const float* scale, const float* shift, int act,
                        const void* res, int res_ld, int res_off, float* stats, void* stream);
/* Stem convolution (yolov8_backbone.py:30-40, the backbone's first Conv(cin, c1, 3, 2, 1), replacing
 * the NHWC input pack + yms_conv_fwd pair): x is the model's NCHW fp32 input [n][cin][h][w], w the
 * fp32 nn.Conv2d weight [cout][cin][3][3] (rounded to s->dtype in the kernel, as the packing
 * does).  Supported: yms_conv_stem_supported(s) (cin 1..3, k 3, stride 2, pad 1, cout % 8 == 0,
 * cout <= 96, bf16 / f16).  Same epilogues as yms_conv_fwd without the residual; statistics:
 * yms_conv_stem_stats_rows(s) rows (one per 8 x 32 output tile), counts after the rows. */
int yms_conv_stem_supported(const yms_conv_shape* s);
int yms_conv_stem_stats_rows(const yms_conv_shape* s);
yms_status yms_conv_stem_fwd(const yms_conv_shape* s, const float* x, const float* w, void* y, int y_ld,
                             int y_off, const float* scale, const float* shift, int act, float* stats,
                             int stats_ld, void* stream);
/* Stem weight gradient with the BN + SiLU backward apply fused in (the stem's dz has no other
 * consumer: the input needs no gradient): dz = scale*(da - coef[c] - (z - mean)*invstd*coef[C+c]),
 * da = gy * SiLU'(z*scale + shift) (act), rounded to s->dtype as the apply pass stores it; then
 * dw[cout][cin][3][3] (+)= sum_pixels dz (x) im2col(x), x the NCHW fp32 input as in
 * yms_conv_stem_fwd.  mean_invstd / coef as yms_bn_act_bwd_apply; ws >= yms_conv_stem_wgrad_ws_bytes. */
size_t yms_conv_stem_wgrad_ws_bytes(const yms_conv_shape* s);
yms_status yms_conv_stem_wgrad(const yms_conv_shape* s, const float* x, const void* gy, int gy_ld, int gy_off,
                               const void* z, int z_ld, int z_off, const float* scale, const float* shift,
                               const float* mean_invstd, const float* coef, int act, float* ws, size_t ws_bytes,
                               float* dw, int accumulate, void* stream);
/* dx (+)= conv_transpose(dz, W) with wpacked_t = yms_conv_pack_weight(.., for_dgrad=1). */
yms_status yms_conv_dgrad(const yms_conv_shape* s, const void* dz, int dz_ld, int dz_off,
                          const void* wpacked_t, void* dx, int dx_ld, int dx_off,
                          int accumulate, void* stream);
/* Input gradient with the PRODUCER's BN + act backward reduce fused into its epilogue: the producer
 * (components.py:69-77 Conv before this one) wrote this conv's input x as act(BN(z)), and this dgrad
 * is the last writer of dx = that producer's output gradient.  dx is stored / accumulated as by
 * yms_conv_dgrad; from the FINAL dx values (as stored) each persistent block writes one partial row
 * ws[r][2][cin] = (sum da, sum da * xhat), da = dx * act'(z*scale + shift), xhat = (z - mean)*invstd
 * (z: view of the dx pixels; scale / shift / mean_invstd as yms_bn_act_bwd_reduce), which replaces
 * the yms_bn_act_bwd_reduce pass: yms_bn_act_bwd_finalize(cin, ws, rows = yms_conv_dgrad_bnred_rows(s), ..).
 * Supported where yms_conv_dgrad_bnred_rows(s) > 0 (the direct 3x3 input-gradient kernel's shapes:
 * 16-bit, 3x3, pad 1, stride 1 or 2, 32 / 64 reduction channels, cin <= 32 and a multiple of 8). */
int yms_conv_dgrad_bnred_rows(const yms_conv_shape* s);
yms_status yms_conv_dgrad_bnred(const yms_conv_shape* s, const void* dz, int dz_ld, int dz_off,
                                const void* wpacked_t, void* dx, int dx_ld, int dx_off, int accumulate,
                                const void* z, int z_ld, int z_off, const float* scale, const float* shift,
                                const float* mean_invstd, int act, float* ws, void* stream);
/* Grouped launches: njobs INDEPENDENT convolutions (host array of jobs, each the arguments of the
 * solo call) in as few launches as their kernels allow.  Jobs that share one kernel variant (dtype,
 * k, epilogue, tile shape, loader) run up to four per launch, every member decomposed exactly as its
 * solo call (same tiles per block, same statistics rows), so every output and statistics row is
 * bit-identical to njobs solo calls; the other jobs (fp32, the direct 3x3 route, stride-2 input
 * gradients, outputs of <= 32 channels, a job alone in its variant) go through the solo call. */
typedef struct {
  yms_conv_shape shape;
  const void* x; int x_ld, x_off;
  const void* wpacked;
  void* y; int y_ld, y_off;
  const float* scale; const float* shift; int act;
  const void* res; int res_ld, res_off;
  float* stats;
} yms_conv_fwd_job;
typedef struct {
  yms_conv_shape shape;
  const void* dz; int dz_ld, dz_off;
  const void* wpacked_t;
  void* dx; int dx_ld, dx_off;
  int accumulate;
} yms_conv_dgrad_job;
yms_status yms_conv_fwd_group(int njobs, const yms_conv_fwd_job* jobs, void* stream);
yms_status yms_conv_dgrad_group(int njobs, const yms_conv_dgrad_job* jobs, void* stream);
/* Host only: the number of calls the grouped call makes for these jobs (grouped launches + solo
 * calls; -1: invalid jobs). */
int yms_conv_fwd_group_launches(int njobs, const yms_conv_fwd_job* jobs);
int yms_conv_dgrad_group_launches(int njobs, const yms_conv_dgrad_job* jobs);
/* dw[cout][cin][k][k] (+)= sum_pixels x (*) dz, fp32; ws = split-K partial slabs. */
size_t yms_conv_wgrad_ws_bytes(const yms_conv_shape* s);
yms_status yms_conv_wgrad(const yms_conv_shape* s, const void* x, int x_ld, int x_off,
                          const void* dz, int dz_ld, int dz_off, float* ws, size_t ws_bytes,
                          float* dw, int accumulate, void* stream);

/* ---- batch norm + activation ---------------------------------------------------------- */
/* Eval: scale = g/sqrt(rv+eps), shift = b - rm*scale (bias-only conv: g=NULL -> scale 1, shift b). */
yms_status yms_bn_fold(int c, const float* gamma, const float* beta, const float* rmean,
                       const float* rvar, float eps, float* scale, float* shift, void* stream);
/* Train: merge the statistics rows of `count` pixels -> mean/invstd, scale/shift, and update the
 * running buffers (unbiased var, momentum) exactly like nn.BatchNorm2d.  mean_invstd: [2][c].
 * Row r = (sum z, sum (z - mean_r)^2) over n_r pixels, n_r = ((float*)stats)[rows*2*stats_ld + r]
 * (the producers' count table; empty rows allowed); rows are merged with Chan's update in fp64.
 * The stats table is consumed: long tables are pre-reduced in place. */
yms_status yms_bn_finalize(int c, float* stats, int rows, int stats_ld, long count,
                           const float* gamma, const float* beta, float* rmean, float* rvar,
                           float momentum, float eps, float* mean_invstd, float* scale,
                           float* shift, void* stream);
/* The same with the invstd row of mean_invstd mi_ld floats after the mean row (>= c): the channel
 * slice of a wider [2][mi_ld] table, for sibling convs whose outputs are slots of one buffer and
 * share one BN backward pass over all their channels (yolov8_head.py:84-85, 99-100). */
yms_status yms_bn_finalize_ld(int c, float* stats, int rows, int stats_ld, long count,
                              const float* gamma, const float* beta, float* rmean, float* rvar,
                              float momentum, float eps, float* mean_invstd, int mi_ld, float* scale,
                              float* shift, void* stream);
/* y = act(z*scale + shift) (+ res), over npix pixels x c channels. */
yms_status yms_affine_act(int dtype, long npix, int c, const void* z, int z_ld, int z_off,
                          const float* scale, const float* shift, int act,
                          const void* res, int res_ld, int res_off,
                          void* y, int y_ld, int y_off, void* stream);
/* Backward of y = silu(bn(z)) (+res):
 *   reduce: partial sums of da and da*xhat (da = gy * silu'(a), a = z*scale+shift) -> ws
 *   finalize: dgamma, dbeta (+=) and the two per-channel coefficients
 *   apply: dz = scale*(da - mean(da) - xhat*mean(da*xhat)), written over dz (may alias z);
 *          gres = gy (gres_acc=0) or gres += gy (gres_acc=1) when gres != NULL (residual). */
int yms_bn_bwd_rows(long npix, int c);   /* partial rows = reduce blocks; ws holds rows*2*c floats */
yms_status yms_bn_act_bwd_reduce(int dtype, long npix, int c, const void* z, int z_ld, int z_off,
                                 const void* gy, int gy_ld, int gy_off, const float* scale,
                                 const float* shift, const float* mean_invstd, int act,
                                 float* ws, void* stream);
yms_status yms_bn_act_bwd_finalize(int c, const float* ws, int rows, long count,
                                   float* dgamma, float* dbeta, float* coef, void* stream);
yms_status yms_bn_act_bwd_apply(int dtype, long npix, int c, const void* z, int z_ld, int z_off,
                                const void* gy, int gy_ld, int gy_off, const float* scale,
                                const float* shift, const float* mean_invstd, const float* coef,
                                int act, void* dz, int dz_ld, int dz_off,
                                void* gres, int gres_ld, int gres_off, int gres_acc, void* stream);
/* reduce + finalize in ONE launch: the last reduce block to finish (agent-scope release/acquire
 * ticket on *counter) sums the partial rows.  *counter must be 0 on entry (it is 0 again on exit);
 * dgamma/dbeta/coef as yms_bn_act_bwd_finalize (any may be NULL). */
yms_status yms_bn_act_bwd_reduce_finalize(int dtype, long npix, int c, const void* z, int z_ld, int z_off,
                                          const void* gy, int gy_ld, int gy_off, const float* scale,
                                          const float* shift, const float* mean_invstd, int act, float* ws,
                                          unsigned* counter, float* dgamma, float* dbeta, float* coef,
                                          void* stream);
/* Bias-only backward of the head's 1x1 nn.Conv2d: dbias = sum over pixels of gy (one launch;
 * counter as above). */
yms_status yms_bias_bwd(int dtype, long npix, int c, const void* gy, int gy_ld, int gy_off,
                        float* ws, unsigned* counter, float* dbias, void* stream);
/* Backward of y = act(z*scale + shift) (+res) where scale / shift fold the RUNNING statistics (a
 * BatchNorm2d in eval mode inside a training step), in ONE launch: gy and z are read once,
 *   da = gy * act'(z*scale + shift), dz = scale * da (dz may alias z), gres as yms_bn_act_bwd_apply;
 *   dbeta = sum da, dgamma = sum da * (z - mean) * invstd with mean_invstd = (running_mean, invstd),
 * summed like yms_bn_act_bwd_reduce_finalize (ws: yms_bn_bwd_rows rows; *counter 0 on entry and on
 * exit; deterministic).  dgamma and dbeta both NULL: a plain streaming pass; mean_invstd, ws and
 * counter are then unused and may be NULL. */
yms_status yms_bn_frozen_act_bwd(int dtype, long npix, int c, const void* z, int z_ld, int z_off,
                                 const void* gy, int gy_ld, int gy_off, const float* scale,
                                 const float* shift, const float* mean_invstd, int act, void* dz, int dz_ld,
                                 int dz_off, void* gres, int gres_ld, int gres_off, int gres_acc, float* ws,
                                 unsigned* counter, float* dgamma, float* dbeta, void* stream);
/* yms_bn_fold plus the table that backward reads: mean_invstd[0][i] = rmean[i], mean_invstd[1][i] =
 * 1/sqrt(rvar[i] + eps), the rows mi_ld floats apart (>= c).  scale / shift are yms_bn_fold's bits.
 * Batched: njobs layers in one launch from a DEVICE table; scale, shift and mean_invstd are byte
 * offsets from base; max_c >= every job's c. */
typedef struct {
  const float* gamma; const float* beta; const float* rmean; const float* rvar;
  float eps; int c, mi_ld;
  long scale, shift, mean_invstd;
} yms_bn_fold_job;
yms_status yms_bn_fold_mi(int c, const float* gamma, const float* beta, const float* rmean, const float* rvar,
                          float eps, float* scale, float* shift, float* mean_invstd, int mi_ld, void* stream);
yms_status yms_bn_fold_mi_batched(int njobs, const yms_bn_fold_job* jobs_dev, int max_c, void* base, void* stream);
/* Grouped forms of the passes above: njobs INDEPENDENT jobs (host array, each the arguments of the solo
 * call), up to eight per launch.  Every member keeps its solo launch's block count and per-block
 * pixel ranges / partial rows, so all outputs are bit-identical to njobs solo calls.  A job alone in
 * the call, a finalize of more than 1024 rows and a reduce without z take the solo call.
 * yms_bn_pass_job serves the four per-pixel passes:
 *   affine:  z, scale, shift, act, res (read, optional) -> out = y
 *   reduce:  z, gy, scale, shift, mean_invstd, act -> ws
 *   apply:   z, gy, scale, shift, mean_invstd, coef, act -> out = dz; res = gres (res_acc), optional
 *   bias:    gy -> dbias (ws, counter as yms_bias_bwd) */
typedef struct {
  int c;
  float* stats; int rows, stats_ld; long count;
  const float* gamma; const float* beta; float* rmean; float* rvar;
  float momentum, eps;
  float* mean_invstd; int mi_ld;
  float* scale; float* shift;
} yms_bn_finalize_job;
typedef struct {
  long npix; int c;
  const void* z; int z_ld, z_off;
  const void* gy; int gy_ld, gy_off;
  const float* scale; const float* shift; const float* mean_invstd; const float* coef;
  int act;
  void* out; int out_ld, out_off;
  void* res; int res_ld, res_off, res_acc;
  float* ws; unsigned* counter; float* dbias;
} yms_bn_pass_job;
typedef struct {
  int c;
  const float* ws; int rows; long count;
  float* dgamma; float* dbeta; float* coef;
} yms_bn_bwd_finalize_job;
yms_status yms_bn_finalize_group(int njobs, const yms_bn_finalize_job* jobs, void* stream);
yms_status yms_affine_act_group(int dtype, int njobs, const yms_bn_pass_job* jobs, void* stream);
yms_status yms_bn_act_bwd_reduce_group(int dtype, int njobs, const yms_bn_pass_job* jobs, void* stream);
yms_status yms_bn_act_bwd_finalize_group(int njobs, const yms_bn_bwd_finalize_job* jobs, void* stream);
yms_status yms_bn_act_bwd_apply_group(int dtype, int njobs, const yms_bn_pass_job* jobs, void* stream);
yms_status yms_bias_bwd_group(int dtype, int njobs, const yms_bn_pass_job* jobs, void* stream);

/* ---- SPPF pools / upsample / layout ---------------------------------------------------- */
/* buf holds 4 consecutive channel slots of width c at channel offset off: slot0 = input x,
 * slots 1..3 <- maxpool5 applied 1,2,3 times (= clipped 5x5 / 9x9 / 13x13 window max). */
yms_status yms_sppf_pool_fwd(int dtype, int n, int h, int w, int c, void* buf, int ld, int off,
                             void* stream);
/* gbuf: grads of the 4 slots; accumulates slot3->slot2->slot1->slot0 through the cascaded
 * pools with PyTorch's first-max argmax (slots 1..2 grads are modified in place). */
size_t yms_sppf_ws_bytes(int n, int h, int w, int c);
yms_status yms_sppf_pool_bwd(int dtype, int n, int h, int w, int c, const void* buf, int ld,
                             int off, void* gbuf, int gld, int goff, void* ws, void* stream);
/* 1 when both entry points above run the shape as one launch with the planes in LDS (16-bit
 * dtypes, h * w within the LDS budget); every other shape runs one launch per pool (forward) or
 * two (backward, which alone uses ws).  Same results either way. */
int yms_sppf_fused_fits(int dtype, int h, int w, int c);
/* Process-wide route for tests and same-tree A/Bs: 0 = always the per-pool launches, 1 = one
 * launch where yms_sppf_fused_fits (the default); a negative v only queries.  Returns the
 * previous value. */
int yms_sppf_route_set(int v);
yms_status yms_upsample2x_fwd(int dtype, int n, int h, int w, int c, const void* x, int x_ld,
                              int x_off, void* y, int y_ld, int y_off, void* stream);
yms_status yms_upsample2x_bwd(int dtype, int n, int h, int w, int c, const void* gy, int gy_ld,
                              int gy_off, void* gx, int gx_ld, int gx_off, int accumulate,
                              void* stream);
/* NCHW fp32 images -> NHWC dtype, channels padded with zeros up to ld. */
yms_status yms_pack_input(int dtype, int n, int c, int h, int w, const float* x, void* y, int ld,
                          void* stream);
/* NHWC view (dtype) <-> NCHW contiguous (dtype_nchw: YMS_F32/BF16/F16). */
yms_status yms_nhwc_to_nchw(int dtype, int dtype_nchw, int n, int h, int w, int c, const void* x,
                            int ld, int off, void* y, void* stream);
yms_status yms_nchw_to_nhwc(int dtype_nchw, int dtype, int n, int h, int w, int c, const void* x,
                            void* y, int ld, int off, int accumulate, void* stream);
/* hipMemsetAsync(p, 0, bytes) / device-to-device hipMemcpyAsync on the stream. */
yms_status yms_zero(void* p, size_t bytes, void* stream);
yms_status yms_copy(void* dst, const void* src, size_t bytes, void* stream);
/* y = cast(x) elementwise (fp32 <-> dtype), count elements. */
yms_status yms_cast(int dtype_in, int dtype_out, long count, const void* x, void* y, void* stream);

/* ---- depthwise k x k conv (YOLO-MS MS-Block inverted bottleneck) --------------- */
/* groups = c, stride 1, pad k/2, k in {3,5,7,9}, c % 8 == 0; w: fp32 [c][k][k] (nn.Conv2d(groups=c)
 * weight, used unpacked).  Not in the reference's code (annotations.md:66-133 diagram only). */
typedef struct {
  int n, h, w, c, k, dtype;
} yms_dw_shape;
/* rows of BN partial statistics written by yms_dwconv_fwd(stats != NULL): one per spatial tile */
int yms_dwconv_stats_rows(const yms_dw_shape* s);
/* stats == NULL: y = act(conv*scale + shift) (scale/shift NULL = identity); else y = conv (pre-BN
 * z) and per-tile (sum z, sum (z - tile mean)^2) rows [rows][2][stats_ld] followed by [rows] pixel
 * counts. */
yms_status yms_dwconv_fwd(const yms_dw_shape* s, const void* x, int x_ld, int x_off, const float* w, void* y,
                          int y_ld, int y_off, const float* scale, const float* shift, int act, float* stats,
                          int stats_ld, void* stream);
/* dx (+)= depthwise conv of dz with the 180-degree rotated kernel */
yms_status yms_dwconv_dgrad(const yms_dw_shape* s, const void* dz, int dz_ld, int dz_off, const float* w, void* dx,
                            int dx_ld, int dx_off, int accumulate, void* stream);
/* dw[c][t] (+)= sum_pixels x(p + d_t) dz(p), fp32, via per-block partials in ws (deterministic) */
size_t yms_dwconv_wgrad_ws_bytes(const yms_dw_shape* s);
yms_status yms_dwconv_wgrad(const yms_dw_shape* s, const void* x, int x_ld, int x_off, const void* dz, int dz_ld,
                            int dz_off, float* ws, size_t ws_bytes, float* dw, int accumulate, void* stream);
/* y (+)= a + b over npix x c channels (b may be NULL); c % 8 == 0 */
yms_status yms_add_views(int dtype, long npix, int c, const void* a, int a_ld, int a_off, const void* b, int b_ld,
                         int b_off, void* y, int y_ld, int y_off, int accumulate, void* stream);
/* Backward of y = a + b in one pass: ga (+)= g, gb (+)= g (acc1 / acc2: accumulate). */
yms_status yms_add_grad2(int dtype, long npix, int c, const void* g, int g_ld, int g_off, void* ga, int ga_ld,
                         int ga_off, int acc1, void* gb, int gb_ld, int gb_off, int acc2, void* stream);

/* ---- mAP@0.5 evaluation (validate_epoch's torchmetrics call, train.py:41-47,146,152-153) ---- */
/* GPU: per image (det_off / gt_off prefix offsets, n_images + 1 entries), rank every detection in
 * its class (stable, score descending), keep the first 100, and greedily match them to the
 * image's ground truths at IoU >= 0.5 (COCOeval semantics) -> tp[d], kept[d] flags.
 * rank_ws: n_det ints of scratch.  max_gt_per_image <= 2048. */
yms_status yms_map_match(int n_images, const float* det_boxes, const float* det_scores, const int* det_labels,
                         const int* det_off, const float* gt_boxes, const int* gt_labels, const int* gt_off,
                         uint8_t* tp, uint8_t* kept, int* rank_ws, int max_gt_per_image, void* stream);
/* HOST (not stream-ordered; host arrays): COCOeval.accumulate at one IoU threshold -> per-class
 * AP (-1 for classes without ground truth) and their mean. */
yms_status yms_map_accumulate(int n_det, const float* scores, const int* labels, const int* image,
                              const uint8_t* tp, const uint8_t* kept, int n_classes, const int* n_gt,
                              double* ap, double* map);
/* ---- COCO AP: mAP@[.5:.95], AP by object size, AR@1/10/100 (torchmetrics' default construction) ---- */
/* GPU: the matching of yms_map_match for n_thr (1..16) increasing IoU thresholds in (0, 1]
 * (iou_thrs: HOST array) times COCOeval's four area ranges all / small / medium / large
 * ([0,1e10], [0,32^2], [32^2,96^2], [96^2,1e10], both ends inclusive), on boxes.  This entry point takes
 * every ground truth as an ordinary one whose area is w*h; yms_map_match_coco_gt below adds COCOeval's
 * iscrowd and annotation area.  Out-of-range ground truths are ignore (visited after the in-range ones,
 * taken only when no in-range one qualifies); a detection matched to one, or unmatched and itself out of
 * range, is ignored.
 *   matched[a * n_det + d], ignored[a * n_det + d]: bit t = at threshold t (area range a)
 *   gt_ignore[g]: bit a = ground truth g is out of area range a
 *   rank_ws: 2 * n_det ints; the first n_det receive the per-class rank (kept = rank < 100)
 * n_det = det_off[n_images].  max_gt_per_image <= 2048 (else YMS_ERR_UNSUPPORTED). */
yms_status yms_map_match_coco(int n_images, int n_det, const float* det_boxes, const float* det_scores,
                              const int* det_labels, const int* det_off, const float* gt_boxes, const int* gt_labels,
                              const int* gt_off, int n_thr, const double* iou_thrs, uint16_t* matched,
                              uint16_t* ignored, uint8_t* gt_ignore, int* rank_ws, int max_gt_per_image,
                              void* stream);
/* GPU: yms_map_match_coco with COCOeval's two per-annotation fields (evaluateImg / computeIoU), indexed
 * like gt_labels, each NULL or given on its own; with both NULL every output byte is yms_map_match_coco's.
 *   gt_area[g] (float, compared as double): the annotation's area -- on COCO the mask's -- decides the
 *     ground truth's area ranges instead of w*h.  The comparisons are the same: a negative area is out of
 *     every range, a NaN inside every one.  A detection's own area stays w*h.
 *   gt_crowd[g] != 0: a crowd (iscrowd) ground truth.  It is ignore in all four ranges and keeps its input
 *     position among its class' ignored ground truths; its IoU with a detection is intersection /
 *     detection area; it is never used up, so any number of detections can match it; a detection whose
 *     best candidate is a crowd is matched and ignored (neither TP nor FP).  An in-range match still wins
 *     over any ignored one, and among equal IoUs the later ground truth.
 *   gt_ignore[g] reports a crowd as out of all four ranges (low bits 1111), so counting the zero bits
 *     gives the non-ignored ground truths unchanged. */
yms_status yms_map_match_coco_gt(int n_images, int n_det, const float* det_boxes, const float* det_scores,
                                 const int* det_labels, const int* det_off, const float* gt_boxes,
                                 const int* gt_labels, const int* gt_off, int n_thr, const double* iou_thrs,
                                 uint16_t* matched, uint16_t* ignored, uint8_t* gt_ignore, int* rank_ws,
                                 int max_gt_per_image, const uint8_t* gt_crowd, const float* gt_area, void* stream);
/* HOST (not stream-ordered; host arrays in evaluation order): COCOeval.accumulate for maxDets
 * 1 / 10 / 100 -> precision[n_thr][101][n_classes][4][3] and recall[n_thr][n_classes][4][3], -1 where
 * npig[class * 4 + area] (the number of non-ignored ground truths) is 0. */
yms_status yms_map_accumulate_coco(int n_det, const float* scores, const int* labels, const int* image,
                                   const int* rank, const uint16_t* matched, const uint16_t* ignored, int n_thr,
                                   int n_classes, const int* npig, double* precision, double* recall);
/* ---- COCO AP on the device: from yms.ops.detect's padded output to the tables, no host read ---- */
/* GPU: the matching of yms_map_match_coco on the padded layout, written into epoch buffers.  Inputs:
 * det_boxes [n_images][max_det][4] xyxy, det_scores / det_labels [n_images][max_det], det_count
 * [n_images] (max_det 1..1024; rows at or beyond an image's count are not read); gt_boxes
 * [n_images][max_gt][4], gt_labels [n_images][max_gt], gt_count [n_images] (max_gt 0..2048, else
 * YMS_ERR_UNSUPPORTED).  A device count above its padded width is clamped to it.  iou_thrs: HOST
 * array, n_thr 1..16, as yms_map_match_coco; n_classes 1..4096.
 * Outputs: epoch buffers of cap rows, of which this call owns [row0, row0 + n_images * max_det) and
 * writes every one: score / label / rank [cap], matched / ignored [4][cap] (area-major, stride cap,
 * bit t = threshold t).  A live row holds its score, its label and exactly yms_map_match_coco's rank
 * and masks for the same image; a dead row (slot >= count) score 0, label -1, rank -1, zero masks.
 *   npig[n_classes][4] += the ground truths of each class that are inside each area range (integer
 *   atomics; a label outside [0, n_classes) is skipped).  The caller zeroes it once per epoch.
 *   order_ws: n_images * max_det ints of scratch. */
yms_status yms_map_match_coco_fixed(int n_images, int max_det, const float* det_boxes, const float* det_scores,
                                    const int* det_labels, const int* det_count, int max_gt, const float* gt_boxes,
                                    const int* gt_labels, const int* gt_count, int n_thr, const double* iou_thrs,
                                    int n_classes, long cap, long row0, float* score, int* label, int* rank,
                                    uint16_t* matched, uint16_t* ignored, int* npig, int* order_ws, void* stream);
/* GPU: the padded-layout matching with yms_map_match_coco_gt's gt_crowd / gt_area, laid out
 * [n_images][max_gt] like gt_labels, each NULL or given on its own (both NULL: yms_map_match_coco_fixed).
 * npig leaves every crowd ground truth out and sorts the others by gt_area where it is given. */
yms_status yms_map_match_coco_fixed_gt(int n_images, int max_det, const float* det_boxes, const float* det_scores,
                                       const int* det_labels, const int* det_count, int max_gt, const float* gt_boxes,
                                       const int* gt_labels, const int* gt_count, int n_thr, const double* iou_thrs,
                                       int n_classes, long cap, long row0, float* score, int* label, int* rank,
                                       uint16_t* matched, uint16_t* ignored, int* npig, int* order_ws,
                                       const uint8_t* gt_crowd, const float* gt_area, void* stream);
/* GPU: yms_map_accumulate_coco over the first n_rows rows of those epoch buffers (cap: the masks'
 * area stride; image = row / max_det, so row order is the host's (image, index) order) -> DEVICE
 * precision[n_thr][101][n_classes][4][3] and recall[n_thr][n_classes][4][3], float64, bit-identical
 * to the host function: a row takes part when 0 <= rank < 100 and 0 <= label < n_classes, within a
 * class the order is (score descending, row ascending).  Stream-ordered, no allocation, no read-back,
 * integer atomics only (the result does not depend on scheduling), and a launch sequence fixed by
 * (n_rows, n_classes).  NaN scores are outside the contract (they sort somewhere; nothing is indexed
 * by them).  ws: yms_map_accumulate_coco_dev_ws_bytes(n_rows, n_thr, n_classes) bytes (never 0),
 * 256-byte aligned; it holds the sort's key / row ping-pong buffers and digit counts. */
size_t yms_map_accumulate_coco_dev_ws_bytes(long n_rows, int n_thr, int n_classes);
yms_status yms_map_accumulate_coco_dev(long n_rows, long cap, const float* score, const int* label, const int* rank,
                                       const uint16_t* matched, const uint16_t* ignored, int n_thr, int n_classes,
                                       const int* npig, double* precision, double* recall, void* ws, size_t ws_bytes,
                                       void* stream);

/* ---- input pipeline ------------------------------------------------------ */
/* dataset.py:132-134 per-sample A.Resize(INTER_LINEAR) + A.Normalize(mean, std) + ToTensorV2 and
 * collate_fn's torch.stack (:260), batched: images = device array of n
 * { const uint8_t* src; int h, w, pitch, flags; } (HWC RGB uint8 rows of `pitch` bytes; flags bit 0
 * horizontal flip, bit 1 vertical flip, applied before the resize); out = [n][3][out_h][out_w] of
 * dtype (YMS_F32 / YMS_BF16 / YMS_F16), (v / 255 - mean[c]) / std[c] (mean, std: host float[3]).
 * cv2 half-pixel bilinear coordinates with edge clamping; fp32 weights (cv2's 8-bit fixed-point
 * rounding is not reproduced). */
yms_status yms_resize_normalize(int dtype, int n, const void* images, int out_h, int out_w, const float* mean,
                                const float* std, void* out, void* stream);
/* The training transform (dataset.py:84-131: HueSaturationValue, Rotate, ShiftScaleRotate, RandomScale,
 * Affine shear, Perspective, flips, then Resize + Normalize + ToTensorV2 + stack), batched: images =
 * device array of n AugImage records (yms_augment_image_bytes() bytes each; layout in
 * csrc/preprocess.hip / yms.data.AugImage): the decoded HWC uint8 source, an optional HSV shift
 * (cv2 8-bit HSV, albumentations LUT semantics) and up to 8 geometric stages, each a 3x3 matrix
 * from its output pixel-index coordinates to its input frame plus that frame's size and border rule
 * (reflect-101 / clamp / constant 0).  The per-image parameters are sampled on the host
 * (yms.data.sample_augmentation); one bilinear sample of the source per output pixel. */
size_t yms_augment_image_bytes(void);
yms_status yms_augment_normalize(int dtype, int n, const void* images, int out_h, int out_w, const float* mean,
                                 const float* std, void* out, void* stream);
/* Mosaic and MixUp (YOLOv5 load_mosaic / random_perspective / mixup, restated; opt-in through
 * yms.data.COCODataset(mosaic=True)), batched: records = device array of n MosImage records
 * (yms_mosaic_image_bytes() bytes each; layout in csrc/preprocess.hip / yms.data.MosImage).  A record
 * is one output image: one or two layers and the MixUp weight r (pixel = b + r * (a - b) before
 * Normalize).  A layer holds a fill value (the canvas background and the constant border), an HSV
 * shift, up to 8 stages with yms_augment_normalize's meaning that end on the canvas, and one to four
 * tiles { src, h, w, pitch, canvas rect, sx, sy, tx, ty }: the canvas coordinate picks the tile whose
 * rect holds its rounded value and samples that tile's source once at (sx * x + tx, sy * y + ty),
 * clamped into the image.  A plain AugImage is the layer with fill 0 and one identity tile, for which
 * the output equals yms_augment_normalize's bit for bit, so mixed batches are one launch. */
size_t yms_mosaic_image_bytes(void);
yms_status yms_mosaic_normalize(int dtype, int n, const void* records, int out_h, int out_w, const float* mean,
                                const float* std, void* out, void* stream);
/* The targets of a batch of sampled plans (yms.data.transform_boxes / mosaic_boxes restated in
 * float64, operation order in csrc/targets.hip), for a loader whose images and annotations stay on
 * the device (yms.cache), opt-in.  boxes / labels: device annotation table, float64 [nann][4] COCO
 * xywh and int32 [nann].  layers: device array of nlayers records (yms_tgt_layer_bytes() each):
 * { int nst, out_w, out_h, pad; double m[8][9] } -- the FORWARD 3x3 stage maps and the output frame.
 * tiles: device array of ntiles records (yms_tgt_tile_bytes() each), sorted by out0:
 * { int image, layer, ann0, count, out0, clip; double gx, gy, ox, oy, rx0, ry0, rx1, ry1 } -- the
 * tile's `count` boxes are annotation rows ann0.., its results are output rows out0..; a box maps to
 * the canvas as (ox + x gx, oy + y gy) and, when clip != 0, is intersected with the rect.
 * out: fp32 [m_cap][6], m_cap = the sum of the counts; EVERY row is written: (image, class, cx, cy, w,
 * h) for a box that survives the filters, (-1, 0, 0, 0, 0, 0) otherwise -- a row the losses ignore.
 * m_cap == 0: YMS_OK, nothing launched. */
size_t yms_tgt_tile_bytes(void);
size_t yms_tgt_layer_bytes(void);
yms_status yms_box_targets(int ntiles, const void* tiles, int nlayers, const void* layers, const double* boxes,
                           const int* labels, long nann, int m_cap, float* out, void* stream);

/* ---- detection loss ------------------------------------------------------- */
/* The reference's ComputeLoss (yolov8/tools/loss.py:94-677; python binding
 * yolov8.tools.loss.ComputeLoss mirrors its constructor and call) on the raw training head maps:
 * maps[l] / grads[l] are NHWC [batch, hs[l], ws_[l], ld] (64 DFL logits, then nc class logits;
 * grads NULL = value only, grads[l] written in full for channels < 64 + nc).  targets: device fp32
 * [n_targets][6] = (image, class, cx, cy, w, h) normalised; boxes scale by (img_w, img_h).
 * iou_type 0 iou, 1 giou, 2 diou, 3 ciou.  pos_weight: NULL or device fp32 [nc].  lambdas (host):
 * box, cls, dfl gains (7.5, 0.5, 1.5 in the reference).  out (device fp32 [4]) = total, box, cls,
 * dfl; grads = d(total)/d(maps).  ws: yms_det_loss_ws_bytes() bytes of device scratch. */
size_t yms_det_loss_ws_bytes(int batch, int anchors, int nc, int n_targets);
yms_status yms_det_loss(int dtype, int batch, int nc, int nlevels, const void* const* maps, void* const* grads,
                        const int* hs, const int* ws_, const float* strides, int ld, const float* targets,
                        int n_targets, float img_w, float img_h, int iou_type, const float* pos_weight,
                        const float* lambdas, void* ws, size_t ws_bytes, float* out, void* stream);
/* bufs[i] (device, dtype, counts[i] elements; 1 <= nbuf <= 4) *= g (device fp32 scalar), in place:
 * the loss's map gradients times the incoming d(out)/d(total) at backward time (replaces
 * `grad * g.to(grad.dtype)` in yolov8/tools/loss.py's autograd backward; a no-op when g == 1). */
yms_status yms_scale_by_device_scalar(int dtype, int nbuf, void* const* bufs, const long* counts, const float* g,
                                      void* stream);

/* ---- task-aligned assigner loss (opt-in; DESIGN.md "Task-aligned loss") --------------------- */
/* YOLOv8's published v8DetectionLoss + TaskAlignedAssigner, restated in tests/tal_ref.py (the
 * definition; parity with the ultralytics package is not pinned).  Arguments as yms_det_loss without
 * iou_type / pos_weight (CIoU, BCE weight 1).  A target row whose image is outside [0, batch) or
 * whose class is outside [0, nc) is ignored.  topk 1..10; alpha, beta >= 0: the exponents of the
 * alignment metric sigmoid(class logit)^alpha * max(CIoU, 0)^beta (published 10, 0.5, 6.0).
 * out (device fp32 [4]) = total, box, cls, dfl with total = batch * (lambdas . terms); grads =
 * d(total)/d(maps).  assign_gt / assign_score: NULL or device [batch * anchors] diagnostics, the
 * target row each anchor is assigned to (-1: background) and its target score. */
size_t yms_tal_loss_ws_bytes(int batch, int anchors, int nc, int n_targets);
yms_status yms_tal_loss(int dtype, int batch, int nc, int nlevels, const void* const* maps, void* const* grads,
                        const int* hs, const int* ws_, const float* strides, int ld, const float* targets,
                        int n_targets, float img_w, float img_h, int topk, float alpha, float beta,
                        const float* lambdas, void* ws, size_t ws_bytes, float* out, int* assign_gt,
                        float* assign_score, void* stream);

/* ---- dynamic soft-label assigner loss (opt-in; DESIGN.md "Dynamic soft-label loss") ---------- */
/* YOLO-MS's own loss (the RTMDet recipe): dynamic soft-label assigner, Quality Focal Loss on the class
 * logits, GIoU on the boxes, both weighted by the matched IoU; restated in tests/dsl_ref.py (the
 * definition; parity with mmdet / mmyolo is not pinned).  Maps, targets, workspace and ignored rows
 * as yms_tal_loss.  topk 1..13: the IoUs summed into a GT's dynamic k; radius, iou_weight >= 0 and
 * beta >= 1, finite: the soft centre prior's radius in strides, the weight of -log(IoU) in the cost and
 * the focal exponent (published 13, 3, 3, 2).  gains (host [3]) = box, cls, dfl gains (published 2, 1;
 * the recipe has no DFL term: 0).  out (device fp32 [5]) = total, box, cls, dfl, norm with total =
 * gains . terms and norm = max(sum of the soft labels, 1); grads = d(total)/d(maps).  assign_gt /
 * assign_score: NULL or device [batch * anchors], the target row each anchor is assigned to (-1:
 * background) and its soft label.  dynamic_k: NULL or device [n_targets], each row's dynamic k (0 for an
 * ignored row and for a row of an image without candidates). */
size_t yms_dsl_loss_ws_bytes(int batch, int anchors, int nc, int n_targets);
yms_status yms_dsl_loss(int dtype, int batch, int nc, int nlevels, const void* const* maps, void* const* grads,
                        const int* hs, const int* ws_, const float* strides, int ld, const float* targets,
                        int n_targets, float img_w, float img_h, int topk, float radius, float iou_weight,
                        float beta, const float* gains, void* ws, size_t ws_bytes, float* out, int* assign_gt,
                        float* assign_score, int* dynamic_k, void* stream);

/* ---- head decode + NMS ------------------------------------------------------------------- */
/* Raw head maps lvl[i]: NHWC [n, h_i, w_i, no_ld] with channels (64 DFL box logits, nc cls
 * logits).  out: [n, A, 4+nc] fp32 = (cx, cy, w, h)*stride_i, sigmoid(cls).  When nms_score
 * is not NULL the NMS prep is fused: boxes_xyxy [n,A,4], score [n,A], label [n,A] (-1 when
 * score <= conf). */
yms_status yms_head_decode(int dtype, int n, int nc, int nlev, const void* const* lvl,
                           const int* hs, const int* ws, int no_ld, const float* strides,
                           float* out, float conf, float* boxes_xyxy, float* nms_score,
                           int* label, void* stream);
/* Standalone DFL integral: x [n][4*ch][A] (dtype) -> out [n][4][A] = sum_j j*softmax_j. */
yms_status yms_dfl(int dtype, int n, int A, int ch, const void* x, void* out, void* stream);
/* Same prep from an already-decoded [n, A, 4+nc] fp32 tensor. */
yms_status yms_nms_prep(int n, int A, int nc, const float* pred, float conf, float* boxes_xyxy,
                        float* score, int* label, void* stream);
/* Class-wise NMS over the prep output.  keep_idx[n][A] (anchor ids), keep_lbl[n][A],
 * counts[n]; per image the kept rows are ordered by class ascending, then by descending
 * score (ties by anchor id), exactly like the reference's per-class torchvision loop.
 * ws: at least yms_nms_ws_bytes_min() bytes; with yms_nms_ws_bytes() bytes (+ ~530 B per anchor
 * of suppressee lists) big sparse-overlap segments may also take the graph kernels.  Every routing
 * gives the same keep lists. */
size_t yms_nms_ws_bytes(int n, int A, int nc);
size_t yms_nms_ws_bytes_min(int n, int A, int nc);
yms_status yms_nms_classwise(int n, int A, int nc, const float* boxes_xyxy, const float* score,
                             const int* label, double iou, int64_t* keep_idx, int* keep_lbl,
                             int* counts, void* ws, size_t ws_bytes, void* stream);
/* Plain torchvision.ops.nms(boxes[m,4], scores[m], iou) on one set -> keep[m], *count. */
yms_status yms_nms_single(int m, const float* boxes, const float* scores, double iou,
                          int64_t* keep, int* count, void* ws, size_t ws_bytes, void* stream);

/* ---- COCO-protocol detect: candidates in front of yms_nms_classwise, finalize behind it --- */
/* The protocol of the published YOLOv8 / YOLO-MS AP (ultralytics non_max_suppression): every
 * (anchor, class) pair above conf, at most K = max_nms of them by score, NMS, at most max_det
 * detections by score, boxes mapped back through the letterbox and clipped.  The tie rules below
 * are this package's (ultralytics leaves ties to its sort: parity UNPINNED).
 *
 * yms_det_candidates: pred [n, A, 4+nc] fp32 (yms_head_decode's out).  multi_label != 0: every pair
 * (a, c) with score > conf (NaN never, +inf does); else per anchor the pair yms_nms_prep picks (max
 * score, ties to the lower class) when its score > conf.  class_mask: NULL or device uint8[nc], 0 =
 * the class is dropped (after the arg-max in best-class mode).  Of an image's candidates the first K
 * by (score descending, anchor ascending, class ascending) survive (a radix select over the score
 * bits; ties at the threshold admitted lowest a * nc + c first) and are stored as rows in ascending
 * a * nc + c: cand_boxes [n][K][4] xyxy (bit-equal to yms_nms_prep's), cand_score, cand_label,
 * cand_anchor [n][K]; unused rows are zero with label and anchor -1.  cand_count[n] = min(count, K),
 * cand_total[n] = the uncapped count.  Bit-exact and independent of block scheduling (integer
 * atomics only); a fixed number of launches, no host read, no allocation: capture-safe.
 * conf >= 0 (negative or NaN: YMS_ERR_INVALID), 1 <= K <= 65536, nc <= 1024, ws of
 * yms_det_ws_bytes() bytes (the NMS workspace is not included), cand_boxes 16-byte aligned.
 * The rows feed yms_nms_classwise(n, K, nc, cand_boxes, cand_score, cand_label, ...) as they are;
 * class-agnostic NMS passes label 0 for every live row with nc = 1 and keeps cand_label aside.
 *
 * yms_det_finalize: of image b's counts[b] kept rows keep_idx[n][K] (yms_nms_classwise's output) the
 * first max_det by (score descending, row ascending) -> det [n][max_det][6] = (x1, y1, x2, y2,
 * score, label from true_label), det_anchor [n][max_det], det_count[n]; rows beyond the count are
 * zero with label and anchor -1.  frames: NULL (boxes pass through) or device fp32 [n][6] =
 * (gain_x, gain_y, pad_x, pad_y, w0, h0): each coordinate becomes min(max((v - pad) / gain, 0), w0
 * or h0), the subtraction and the division separately rounded.  1 <= max_det <= 1024. */
size_t yms_det_ws_bytes(int n, int A, int nc, int K);
yms_status yms_det_candidates(int n, int A, int nc, const float* pred, float conf, int multi_label,
                              const uint8_t* class_mask, int K, float* cand_boxes, float* cand_score,
                              int* cand_label, int* cand_anchor, int* cand_count, int* cand_total, void* ws,
                              size_t ws_bytes, void* stream);
yms_status yms_det_finalize(int n, int K, int max_det, const float* cand_boxes, const float* cand_score,
                            const int* true_label, const int* cand_anchor, const int64_t* keep_idx,
                            const int* counts, const float* frames, float* det, int* det_anchor, int* det_count,
                            void* stream);

/* ---- test-time augmentation: view merge in front of yms_det_candidates, box voting behind the NMS ---- */
/* Nothing in the reference.  The multi-view protocols of the published numbers (ultralytics
 * augment=True: scales 1 / 0.83 / 0.67 with a left-right flip on the middle view; the RTMDet-lineage
 * tta_model: 3 sizes x flip) de-flip and de-scale every view's predictions, concatenate them and run
 * one NMS; ultralytics' merge=True then replaces each kept box by the score-weighted mean of the boxes
 * around it.  Semantics and tie rules are this package's (parity with ultralytics / mmyolo UNPINNED).
 *
 * yms_tta_merge: nviews in 1..YMS_TTA_MAX_VIEWS decoded predictions preds[v] [n, A[v], 4+nc] fp32
 * (yms_head_decode's out; boxes (cx, cy, w, h) in view pixels) -> out [n, R, 4+nc], R = sum of
 * a1[v] - a0[v]: view v's rows [a0[v], a1[v]) in call order, ascending inside a view (merged row
 * roff_v + (a - a0[v]) with roff_v the prefix sum of the earlier views' row counts).  H[v] x W[v] is the
 * view's input size, flips[v] bit 0 = the input was flipped left-right, bit 1 = up-down
 * (yms_resize_normalize's bits), frames[v] device fp32 [n][6] = (gain_x, gain_y, pad_x, pad_y, w0,
 * h0) of the view's letterbox per image.  Per row, each operation separately rounded in fp32:
 *   x = (flip & 1) ? (float)W - cx : cx;   y = (flip & 2) ? (float)H - cy : cy;
 *   cx0 = (x - pad_x) / gain_x;  cy0 = (y - pad_y) / gain_y;  w0 = w / gain_x;  h0 = h / gain_y
 * Nothing is clipped; the nc scores are copied bit for bit (a NaN keeps its payload); a NaN or
 * infinite box number or a zero gain propagates by IEEE rules.  The arrays preds, A, a0, a1, H, W,
 * flips and frames are HOST arrays of nviews entries, read during the call (they travel as kernel
 * arguments: no device table).  One launch, no host read of device memory, no allocation:
 * capture-safe.  YMS_ERR_INVALID: nviews outside 1..8, a NULL pointer, an empty range or one outside
 * [0, A[v]], a flip outside 0..3, a size < 1, n outside 1..65535, nc < 1, a view with A[v] * (4+nc) >= 2^31, or R * nc >= 2^31.  Any
 * nc >= 1 (rows of 4+nc floats need only 4-byte alignment; 16-byte loads are used when 4+nc is a
 * multiple of 4 and every base is 16-byte aligned).  out must not overlap an input.
 *
 * yms_det_finalize_vote: yms_det_finalize's contract with the same selection, scores, labels,
 * anchors, counts, fill rows, frames un-map and clip; only the box of each emitted row i differs,
 * taken before the un-map:
 *   M_i   = { live rows j < cand_count[b] : nms_label[j] == nms_label[i] and (double)ovr(i, j) > iou }
 *   box_i = sum_{j in M_i} score_j box_j / sum_{j in M_i} score_j   (float64 sums, one rounding to fp32)
 * ovr is yms_nms_classwise's own fp32 expression (inter / (area_i + area_j - inter), areas (x2-x1)*(y2-y1),
 * inter = max(0, xx2-xx1) * max(0, yy2-yy1)), evaluated by the same device function.  nms_label [n][K]
 * is the label array that was handed to yms_nms_classwise (all zero on live rows for class-agnostic
 * NMS), cand_count[n] yms_det_candidates' count.  A row whose score sum is 0 or not finite keeps
 * its own box: that covers an empty M_i (a zero-area box: its ovr with itself is NaN; iou >= 1) and
 * a +inf score.  A NaN overlap never makes a member.  The float64 summation order is fixed, so the
 * output is deterministic; it is specified to one fp32 ulp of the exactly rounded mean, not bit for
 * bit.  Ties in the selection as yms_det_finalize.  Two launches (det's box slots carry the row ids
 * from the first to the second), no host read, no allocation: capture-safe.  YMS_ERR_INVALID as
 * yms_det_finalize, and for a NULL cand_count / nms_label, a NaN iou or n > 65535. */
#define YMS_TTA_MAX_VIEWS 8
yms_status yms_tta_merge(int n, int nc, int nviews, const float* const* preds, const int* A, const int* a0,
                         const int* a1, const int* H, const int* W, const int* flips,
                         const float* const* frames, float* out, void* stream);
yms_status yms_det_finalize_vote(int n, int K, int max_det, const float* cand_boxes, const float* cand_score,
                                 const int* true_label, const int* cand_anchor, const int64_t* keep_idx,
                                 const int* counts, const float* frames, const int* cand_count,
                                 const int* nms_label, double iou, float* det, int* det_anchor, int* det_count,
                                 void* stream);

/* ---- tiled inference of large images: the tiles' merge in front of yms_det_candidates ---------------- */
/* Nothing in the reference.  Sliced inference (popularised by SAHI) cuts a large image into overlapping
 * tiles at native resolution, runs every tile, maps each tile's predictions back and runs one NMS over
 * all of them.  The grid and suppression rules are this package's (yms/tiles.py; parity with SAHI
 * UNPINNED); this entry point is the gather.
 *
 * yms_tile_merge: pred [T, A, 4+nc] fp32, the decoded predictions (yms_head_decode's out; boxes (cx, cy,
 * w, h) in tile-input pixels) of T tile inputs of one common size -> out [n, S * A, 4+nc] in
 * original-image pixels.  table: DEVICE array of n * S yms_tile_slot records, record b * S + s being
 * slot s of image b, which owns out's rows [s * A, (s + 1) * A) of image b, row s * A + a from row a of
 * pred[tile].  S is the largest slot count of any image; an image with fewer leaves slots empty.
 *   live slot (0 <= tile < T), per row, each operation separately rounded in fp32 (no contraction):
 *     cx0 = (cx - pad_x) / gain_x;  cy0 = (cy - pad_y) / gain_y;  w0 = w / gain_x;  h0 = h / gain_y
 *     the row is SUPPRESSED when  cx - 0.5f * w < lo_x  or  cy - 0.5f * h < lo_y  or
 *     cx + 0.5f * w > hi_x  or  cy + 0.5f * h > hi_y  (tile-input pixels, strict comparisons: a side
 *     on its bound stays; a NaN coordinate or bound suppresses nothing; -inf / +inf disables a side).
 *     A suppressed row's box is un-mapped as usual and each of its nc scores is written as -1.0f; any
 *     other row's scores are copied bit for bit (a NaN keeps its payload).  Nothing is clipped.
 *   empty slot (tile == -1), and any tile outside [0, T): four zeros and nc scores of -1.0f.  The table
 *     is device data that the host cannot see: the kernel checks the index and never reads outside pred.
 * yms_det_candidates takes a pair only for score > conf with conf >= 0, so a -1 row is never a
 * candidate, a kept detection or a voter; that is the whole suppression mechanism.
 * One launch, no host read of device memory, no allocation: capture-safe.  YMS_ERR_INVALID: a NULL or
 * not 4-byte aligned pointer, n outside 1..65535, S, A, nc or T < 1, A * (4+nc) > 2^31 - 1, or
 * S * A * nc >= 2^31 (yms_det_candidates' limit on the merged rows).  Any nc >= 1: 16-byte accesses are
 * used when 4+nc is a multiple of 4 and pred and out are 16-byte aligned, single floats otherwise.  out
 * must not overlap pred or the table.  The launch has at most yms_tile_merge_max_blocks() blocks, each
 * striding over (slot, 256-unit chunk) work items. */
typedef struct {
  int32_t tile;                          /* index into pred's first axis; -1 = empty slot */
  float gain_x, gain_y, pad_x, pad_y;    /* orig = (v - pad) / gain for centres, v / gain for w, h */
  float lo_x, lo_y, hi_x, hi_y;          /* suppression bounds in tile-input pixels */
  int32_t reserved[3];                   /* 48-byte records; ignored */
} yms_tile_slot;
int yms_tile_merge_max_blocks(void);
yms_status yms_tile_merge(int n, int S, int A, int nc, int T, const float* pred, const yms_tile_slot* table,
                          float* out, void* stream);

/* ---- optimizer step: SGD / Adam + weight EMA + norm clipping + non-finite skip ------------ */
/* Replaces torch.optim.SGD / Adam behind tools/utils.py:11-25 get_optimizer, the
 * torch.isnan(loss) + loss.item() guard of train.py:365,376, and the ModelEMA / clip_grad_norm_
 * every YOLOv8 recipe adds, in a launch count that does not depend on the number of tensors: the
 * tensors are described by a device table of fixed-size chunks instead of kernel arguments.
 *
 * A job is one fp32 tensor of `count` >= 1 elements.  param: its device address (16-B alignment is
 * used when present, 4-B is enough).  grad: the gradient as a byte offset from the grad_base given
 * per call (the flat gradient arena), or an absolute address (YMS_OPTIM_GRAD_ABS), or none
 * (YMS_OPTIM_GRAD_NONE: no update; the EMA, if any, still follows the tensor).  state0 / state1 / ema:
 * ELEMENT offsets of the job's slots in the three flat fp32 buffers given to
 * yms_optim_table_build (momentum | exp_avg, exp_avg_sq, EMA), -1 = no slot.  An update needs
 * state0 (and state1 for Adam); YMS_OPTIM_EMA needs ema >= 0.  group: index into the hyper array. */
#define YMS_OPTIM_SGD 0
#define YMS_OPTIM_ADAM 1
#define YMS_OPTIM_GRAD_NONE 1
#define YMS_OPTIM_GRAD_ABS 2
#define YMS_OPTIM_EMA 4
#define YMS_OPTIM_MAX_GROUPS 8
typedef struct {
  void* param;
  int64_t grad;
  int64_t state0, state1, ema;
  int64_t count;
  int group, flags;
} yms_optim_job;
/* One row of the device table: at most yms_optim_chunk_elems() consecutive elements of ONE job, so a
 * block's work does not depend on which tensor it lands in.  All addresses are absolute but g,
 * which keeps the job's meaning (offset of the chunk's first gradient element, or its address). */
typedef struct {
  float* p;
  int64_t g;
  float* s0;
  float* s1;
  float* e;
  int n;
  short group, flags;
} yms_optim_chunk;
/* Device arrays the step reads (never kernel arguments, so a captured graph sees a new value):
 * max_norm <= 0 = no clipping; skip_nonfinite != 0 = write nothing when the norm is not finite;
 * ema_decay / ema_tau: delta = decay * (1 - exp(-k / tau)), tau <= 0 = the plain decay;
 * group[i] = { lr, momentum | beta1, beta2, eps, weight_decay, nesterov != 0, 0, 0 }.  Doubles, as
 * torch holds them: 1 - beta2 taken from a float 0.999 is already off in the fifth digit. */
typedef struct {
  double max_norm, skip_nonfinite, ema_decay, ema_tau;
  double group[YMS_OPTIM_MAX_GROUPS][8];
} yms_optim_hyper;
typedef struct {
  int step, ema_step, skipped;   /* updates applied, EMA updates applied, steps skipped */
  float grad_norm;               /* the last step's gradient norm (with partials) */
} yms_optim_counters;
/* HOST only (no launch): elements per chunk; rows / bytes of the table of a job list (-1 / 0: invalid
 * jobs); the table itself into caller-owned HOST memory (the caller uploads it; it holds no gradient
 * address in the offset form, so one table serves every arena and is valid inside a captured
 * graph); and the number of partial sums yms_optim_grad_norm writes for a table of nchunks rows. */
int yms_optim_chunk_elems(void);
long yms_optim_table_chunks(int njobs, const yms_optim_job* jobs);
size_t yms_optim_table_bytes(int njobs, const yms_optim_job* jobs);
yms_status yms_optim_table_build(int njobs, const yms_optim_job* jobs, float* state0, float* state1, float* ema,
                                 void* table, size_t table_bytes);
int yms_optim_norm_partials(long nchunks);
/* partials[yms_optim_norm_partials(nchunks)] <- sums of squares of the table's gradients: one
 * launch, no atomics, a fixed summation tree (bit-reproducible; no chain of more than 128 sequential
 * fp32 additions). */
yms_status yms_optim_grad_norm(const void* table, long nchunks, const void* grad_base, float* partials,
                               void* stream);
/* One optimizer step in two launches (the update over the table, then a one-block tick that advances
 * the counters and stores the norm).  fp32 arithmetic as torch.optim; the bias corrections and the
 * EMA factor in fp64 from the device counters:
 *   SGD   d = g + wd p;  b' = d (first update) | mom b + d;  p' = p - lr (nesterov ? d + mom b' : b')
 *   Adam  d = g + wd p;  m' = b1 m + (1-b1) d;  v' = b2 v + (1-b2) d^2;
 *         p' = p - (lr / bc1) m' / (sqrt(v') / sqrt(bc2) + eps),  bc_i = 1 - b_i^t   (no amsgrad; AdamW: below)
 *   EMA   e' = delta e + (1 - delta) p'
 * partials != NULL (npartials of yms_optim_grad_norm's sums): every block re-reduces them in one
 * fixed order, scales g by min(1, max_norm / (norm + 1e-6)) (torch's clip_grad_norm_) and, when the
 * norm is not finite and skip_nonfinite is set, writes nothing (the tick then counts a skipped step). */
yms_status yms_optim_step(int kind, const void* table, long nchunks, const void* grad_base,
                          const yms_optim_hyper* hyper, yms_optim_counters* counters, const float* partials,
                          int npartials, void* stream);
/* The same step with a third update kind, a second EMA rule and a schedule evaluated on the device.
 * yms_optim_step is this call with ext = sched_out = NULL (bit-identical) and kinds 0 / 1 only.
 *   AdamW (kind 2)  d = g clip (no wd p term);  p1 = p * (float)(1 - lr wd), the factor formed in fp64;
 *         m', v' as Adam's from d;  p' = p1 - (lr / bc1) m' / (sqrt(v') / sqrt(bc2) + eps)
 *         (torch.optim.AdamW without amsgrad; the hyper row is Adam's).
 * ext (a DEVICE record like hyper, may be NULL = today's EMA rule, no schedule):
 *   ema_rule YMS_OPTIM_EMA_EXPMOM: mu = (1 - m) exp(-(k + 1) / gamma) + m at ema_step k (gamma <= 0:
 *         mu = m), e' = (1 - mu) e + mu p', with m = hyper->ema_decay and gamma = hyper->ema_tau.
 *   seg[0 .. nsegments): the schedule.  Its index is n = counters->step + counters->skipped, the
 *         number of calls before this one (a skipped step advances it).  Segment s is the factor
 *         from (n <= begin), to (n >= end), else with u = (n - begin) / (end - begin)
 *         linear from + (to - from) u | cosine to + (from - to)(1 + cos(pi u)) / 2.  Group g runs at
 *         group[g][0] times the product of the factors of the YMS_OPTIM_SCHED_LR segments whose
 *         `groups` has bit g, and at group[g][1] (SGD momentum / Adam beta1, whose 1 - beta1 and bias
 *         correction follow it) times that of the YMS_OPTIM_SCHED_MOMENTUM ones: fp64, before the
 *         casts to float.  The record is never read by the host: nsegments is clamped to
 *         [0, YMS_OPTIM_MAX_SEGMENTS] and a segment with end <= begin or an unknown target or shape
 *         is ignored, by the kernel.
 * sched_out (device, [YMS_OPTIM_MAX_GROUPS][2], may be NULL): the tick stores { lr, momentum | beta1 }
 * as this call used them, for logging without a sync.  Launch count as yms_optim_step. */
#define YMS_OPTIM_ADAMW 2
#define YMS_OPTIM_EMA_TAU 0
#define YMS_OPTIM_EMA_EXPMOM 1
#define YMS_OPTIM_SCHED_LR 0
#define YMS_OPTIM_SCHED_MOMENTUM 1
#define YMS_OPTIM_SCHED_LINEAR 0
#define YMS_OPTIM_SCHED_COSINE 1
#define YMS_OPTIM_MAX_SEGMENTS 8
typedef struct {
  double begin, end, from, to;
  int target, shape, groups, pad;   /* groups: bit g = group g */
} yms_optim_segment;
typedef struct {
  double ema_rule;
  double nsegments;
  yms_optim_segment seg[YMS_OPTIM_MAX_SEGMENTS];
} yms_optim_ext;
yms_status yms_optim_step_ext(int kind, const void* table, long nchunks, const void* grad_base,
                              const yms_optim_hyper* hyper, const yms_optim_ext* ext, yms_optim_counters* counters,
                              double* sched_out, const float* partials, int npartials, void* stream);
/* Exchange every YMS_OPTIM_EMA row's tensor with its EMA slot, in place, in one launch. */
yms_status yms_optim_swap(const void* table, long nchunks, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* YMS_H */
