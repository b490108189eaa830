// Implicit-GEMM convolution for gfx950 (MI355X) on MFMA, NHWC activations.
//
// Replaces the reference's Conv = Conv2d(bias=False) -> BatchNorm2d -> SiLU
// (yolov8/model/components.py:69-77), its residual add (Bottleneck, :87-93), the channel
// concatenations feeding C2f/SPPF/neck/head (:119, :146; yolov8_neck.py:79-91;
// yolov8_head.py:122 -- producers write at a channel offset of the consumer's buffer),
// the head's biased 1x1 nn.Conv2d (yolov8_head.py:86-109) and the autograd of all of them.
//
// GEMM views (rows = pixels, 16-B "chunks" of 8 bf16/f16 or 4 f32 channels along K):
//   forward : Y[pix][co]  = sum_{tap,ci} X[src(pix,tap)][ci] * W[co][tap,ci]      (NT)
//   dgrad   : DX[pix][ci] = sum_{tap,co} DZ[src'(pix,tap)][co] * W[co][ci][tap]    (NT)
// NT tiles are staged global->regs->LDS as [rows][64 B of K] (80-B padded pitch, bank-
// conflict-free for ds_read_b128) and consumed by v_mfma_f32_32x32x16_{bf16,f16}
// (or v_mfma_f32_32x32x2_f32 for the exact-fp32 path).  The weight gradient is wgrad.hip.
#include <algorithm>
#include <vector>

#include "conv_common.hpp"
#include "conv_direct.hpp"

namespace yms {

struct NTParams {
  const char* src;
  const char* wp;
  char* dst;
  int src_ld, src_off, dst_ld, dst_off;
  const float* scale;
  const float* shift;
  int act;
  const char* res;
  int res_ld, res_off;
  float* stats;
  int stats_ld;
  float* stats_cnt; // per-row pixel counts (right after the rows, conv_common.hpp contract)
  int SH, SW;       // source spatial dims
  int OW;           // row-space width
  int stride, pad;
  int cpt;          // 16-B chunks per tap along source channels
  uint64_t cpt_magic;   // kc / cpt == (kc * cpt_magic) >> 32 for every kc < nkt * 8 (host-checked)
  uint32_t src_bytes;   // byte extent of the source view's buffer (raw-buffer num_records, < 2^31)
  int Kc;           // valid K chunks
  int nkt;          // K tiles (4 chunks each)
  int M;            // rows (pixels)
  int Ncols;        // valid output columns
  int tiles_n;
  FastDiv div_ow, div_ohw;
  // MODE_DGRAD2: one GEMM per output-parity class (ry, rx) = (blockIdx.y >> 1, blockIdx.y & 1).
  // Class rows are the dx pixels (n, 2a+ry, 2b+rx); its taps are kh = kh0 + 2*jy, kw = kw0 + 2*jx,
  // reading dz at (a + c0y - jy, b + c0x - jx); weights are packed per class.
  int OH, OWx;                      // dx spatial dims (for the output pixel index)
  int cls_M[4], cls_nkt[4], cls_Kc[4], cls_ntx[4], cls_c0y[4], cls_c0x[4];
  long cls_woff[4];                 // byte offset of the class' packed weight block
  FastDiv cls_div_w[4], cls_div_hw[4];
};

// 16-B zero chunk: out-of-image / out-of-K im2col lanes load from here, so the A loads are
// branch-free (no exec-masked regions around each global load).
__device__ __attribute__((aligned(64))) u32x4 g_zero_chunk[4];

// 16-bit types (GL): k-tiles are staged global->LDS directly with global_load_lds_dwordx4 into
// an ST-deep ring of unpadded 128-B rows; 16-B chunk c of row r lives in slot
// c ^ ((r >> 1) & 7) (conflict-free ds_read_b128 for 16 consecutive rows), which is realised
// by swizzling each lane's global SOURCE address since the LDS image of one wave-instruction is
// lane-linear.  The wait for k-tile kt is a counted vmcnt that leaves ST-2 later tiles in
// flight across a raw s_barrier.  fp32 keeps the register-staged double buffer.
template <typename T, int KS, int MODE, int EPI, int BM, int BN, int WGM, int WGN, int ST>
__global__ __launch_bounds__(256, 2) void conv_nt_kernel(NTParams p) {
  constexpr int WTM = BM / WGM, WTN = BN / WGN;
  constexpr int TM = WTM / 32, TN = WTN / 32;
  constexpr int RSTEP = 256 / NT_KCH;                      // rows covered by one load pass
  constexpr int A_SLOTS = BM / RSTEP;
  constexpr int B_CHUNKS = BN * NT_KCH;
  constexpr int B_SLOTS = (B_CHUNKS + 255) / 256;
  constexpr bool F32 = sizeof(T) == 4;
  constexpr bool GL = !F32;
  constexpr int PITCH = GL ? 128 : NT_ROWP;
  constexpr int NSTAGE = GL ? ST : 2;
  constexpr int TILE_BYTES = (BM + BN) * PITCH;
  constexpr int EPI_P = BN + 4;                            // fp32 staging pitch (floats)
  constexpr int SMEM = (NSTAGE * TILE_BYTES > BM * EPI_P * 4) ? NSTAGE * TILE_BYTES : BM * EPI_P * 4;
  static_assert(!GL || B_CHUNKS % 256 == 0, "GL loader needs whole B passes");
  static_assert(TM >= 1 && TN >= 1 && A_SLOTS >= 1, "bad tile");
  __shared__ __attribute__((aligned(16))) char smem[SMEM];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WGN, wn = wave % WGN;
  const int wg = xcd_remap(blockIdx.x, gridDim.x);
  const int tile_n = wg % p.tiles_n, tile_m = wg / p.tiles_n;
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  int M = p.M, nkt = p.nkt, Kc = p.Kc, ntx = 1, cls = 0;
  const char* wp = p.wp;
  FastDiv dv_w = p.div_ow, dv_hw = p.div_ohw;
  if (MODE == MODE_DGRAD2) {
    cls = blockIdx.y;
    M = p.cls_M[cls];
    nkt = p.cls_nkt[cls];
    Kc = p.cls_Kc[cls];
    ntx = p.cls_ntx[cls];
    wp = p.wp + p.cls_woff[cls];
    dv_w = p.cls_div_w[cls];
    dv_hw = p.cls_div_hw[cls];
    if (m0 >= M) return;   // uniform: this class has fewer row tiles
  }

  // ---- im2col loader state (A side): fixed chunk column q, rows r0 + RSTEP*i ----
  // (GL: the thread fills LDS slot tid&7 of rows r0 + 32i, i.e. chunk (tid&7) ^ ((tid>>4)&7))
  const int q = GL ? ((tid & 7) ^ ((tid >> 4) & 7)) : (tid & (NT_KCH - 1)), r0 = tid / NT_KCH;
  // Per row slot: the element offset of its tap-(0,0) source pixel (32-bit; the host checks
  // the source fits) and a bit mask of the taps that land inside the image.  Per k-tile the
  // A address is then offset + delta(tap) + channel chunk, with no per-tap bounds arithmetic.
  // Tap t displaces the source pixel by (dy, dx): forward (+t/KS, +t%KS); stride-1 dgrad
  // (-t/KS, -t%KS); stride-2 dgrad parity class (-jy, -jx).
  constexpr int NTAPS = MODE == MODE_DGRAD2 ? 4 : KS * KS;
  constexpr int SGN = MODE == MODE_FWD ? 1 : -1;
  auto tap_dyx = [&](int t, int& dy, int& dx) {
    if (MODE == MODE_DGRAD2) {
      dy = ntx == 1 ? t : (t >> 1);
      dx = ntx == 1 ? 0 : (t & 1);
    } else {
      dy = t / KS;
      dx = t - (t / KS) * KS;
    }
  };
  int a_off[A_SLOTS];
  uint32_t a_msk[A_SLOTS];
#pragma unroll
  for (int i = 0; i < A_SLOTS; ++i) {
    const int m = m0 + r0 + RSTEP * i;
    const bool row_ok = m < M;
    const uint32_t mm = row_ok ? (uint32_t)m : 0u;
    const uint32_t n = fdiv(mm, dv_hw);
    const uint32_t rem = mm - n * dv_hw.d;
    const uint32_t oy = fdiv(rem, dv_w);
    const uint32_t ox = rem - oy * dv_w.d;
    int y0, x0;
    if (MODE == MODE_FWD) {
      y0 = (int)oy * p.stride - p.pad;
      x0 = (int)ox * p.stride - p.pad;
    } else if (MODE == MODE_DGRAD) {
      y0 = (int)oy + p.pad;
      x0 = (int)ox + p.pad;
    } else {
      y0 = (int)oy + p.cls_c0y[cls];
      x0 = (int)ox + p.cls_c0x[cls];
    }
    a_off[i] = (((int)n * p.SH + y0) * p.SW + x0) * p.src_ld + p.src_off;
    uint32_t msk = 0;
#pragma unroll
    for (int t = 0; t < NTAPS; ++t) {
      int dy, dx;
      tap_dyx(t, dy, dx);
      const int iy = y0 + SGN * dy, ix = x0 + SGN * dx;
      if (row_ok && iy >= 0 && iy < p.SH && ix >= 0 && ix < p.SW) msk |= 1u << t;
    }
    a_msk[i] = msk;
  }
  int tap = q / p.cpt, cc = q - (q / p.cpt) * p.cpt;
  constexpr int EPC = 16 / (int)sizeof(T);   // elements per 16-B chunk

  u32x4 a_reg[A_SLOTS], b_reg[B_SLOTS];

  // GL: buf = ring stage to fill with LDS-DMA; register path: buf unused (a_reg/b_reg)
  auto load_tile = [&](int kt, int buf) {
    char* lds_a = smem + buf * TILE_BYTES + wave * 1024;
    char* lds_b = smem + buf * TILE_BYTES + BM * PITCH + wave * 1024;
    (void)lds_a; (void)lds_b;
    const int kc = kt * NT_KCH + q;
    const bool kok = kc < Kc;
    int dy, dx;
    tap_dyx(tap, dy, dx);
    const int delta = SGN * (dy * p.SW + dx) * p.src_ld + cc * EPC;
    const uint32_t tbit = 1u << (tap & 31);
#pragma unroll
    for (int i = 0; i < A_SLOTS; ++i) {
      const bool ok = kok && (a_msk[i] & tbit);
      const char* ap = ok ? p.src + (long)(a_off[i] + delta) * (long)sizeof(T)
                          : reinterpret_cast<const char*>(g_zero_chunk);
      if constexpr (GL) glds16(ap, lds_a + i * 256 * 16);
      else a_reg[i] = *reinterpret_cast<const u32x4*>(ap);
    }
#pragma unroll
    for (int j = 0; j < B_SLOTS; ++j) {
      const int c = tid + 256 * j;
      if (B_CHUNKS >= 256 * (j + 1) || c < B_CHUNKS) {
        const int row = c / NT_KCH, qq = GL ? q : c % NT_KCH;   // GL: swizzled source chunk
        const long off = ((long)(n0 + row) * (nkt * NT_KCH) + kt * NT_KCH + qq) * 16;
        if constexpr (GL) glds16(wp + off, lds_b + j * 256 * 16);
        else b_reg[j] = *reinterpret_cast<const u32x4*>(wp + off);
      }
    }
    // advance the tap cursor by one k-tile of chunks
    cc += NT_KCH;
    while (cc >= p.cpt) { cc -= p.cpt; ++tap; }
  };

  auto store_tile = [&](int buf) {
    char* A = smem + buf * TILE_BYTES;
    char* B = A + BM * NT_ROWP;
#pragma unroll
    for (int i = 0; i < A_SLOTS; ++i)
      *reinterpret_cast<u32x4*>(A + (r0 + RSTEP * i) * NT_ROWP + q * 16) = a_reg[i];
#pragma unroll
    for (int j = 0; j < B_SLOTS; ++j) {
      const int c = tid + 256 * j;
      if (B_CHUNKS >= 256 * (j + 1) || c < B_CHUNKS)
        *reinterpret_cast<u32x4*>(B + (c / NT_KCH) * NT_ROWP + (c % NT_KCH) * 16) = b_reg[j];
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
  // The whole 128-B k-tile is always computed: chunks beyond K are zero on both sides (A
  // loads the zero chunk, packed weights are zero-padded), so no branches split the MFMA
  // stream and the fragment reads of substep s+1 overlap the MFMAs of substep s.
  auto compute = [&](int buf) {
    const char* A = smem + buf * TILE_BYTES;
    const char* B = A + BM * PITCH;
    if constexpr (!F32) {
      u32x4 af[2][TM], bfr[2][TN];
      const int swz = (lr >> 1) & 7;   // rows of a fragment differ from lr by multiples of 16
      auto frags = [&](int s, int slot) {
        const int co = ((2 * s + lh) ^ swz) * 16;
#pragma unroll
        for (int a = 0; a < TM; ++a)
          af[slot][a] = *reinterpret_cast<const u32x4*>(A + (wm * WTM + a * 32 + lr) * PITCH + co);
#pragma unroll
        for (int b = 0; b < TN; ++b)
          bfr[slot][b] = *reinterpret_cast<const u32x4*>(B + (wn * WTN + b * 32 + lr) * PITCH + co);
      };
      frags(0, 0);
#pragma unroll
      for (int s = 0; s < NT_KCH / 2; ++s) {
        if (s + 1 < NT_KCH / 2) frags(s + 1, (s + 1) & 1);
#pragma unroll
        for (int a = 0; a < TM; ++a)
#pragma unroll
          for (int b = 0; b < TN; ++b) acc[a][b] = Mfma<T>::mma(af[s & 1][a], bfr[s & 1][b], acc[a][b]);
      }
    } else {
      // fp32: per 64-B substep lane (r,h) holds k = 8h..8h+7; MFMA j pairs element j of both halves.
#pragma unroll
      for (int s = 0; s < NT_KCH / 4; ++s) {
        {
          float af[TM][8], bfr[TN][8];
#pragma unroll
          for (int a = 0; a < TM; ++a) {
            const float4* src = reinterpret_cast<const float4*>(A + (wm * WTM + a * 32 + lr) * NT_ROWP + 64 * s + 32 * lh);
            float4 u = src[0], v = src[1];
            af[a][0] = u.x; af[a][1] = u.y; af[a][2] = u.z; af[a][3] = u.w;
            af[a][4] = v.x; af[a][5] = v.y; af[a][6] = v.z; af[a][7] = v.w;
          }
#pragma unroll
          for (int b = 0; b < TN; ++b) {
            const float4* src = reinterpret_cast<const float4*>(B + (wn * WTN + b * 32 + lr) * NT_ROWP + 64 * s + 32 * lh);
            float4 u = src[0], v = src[1];
            bfr[b][0] = u.x; bfr[b][1] = u.y; bfr[b][2] = u.z; bfr[b][3] = u.w;
            bfr[b][4] = v.x; bfr[b][5] = v.y; bfr[b][6] = v.z; bfr[b][7] = v.w;
          }
#pragma unroll
          for (int j = 0; j < 8; ++j)
#pragma unroll
            for (int a = 0; a < TM; ++a)
#pragma unroll
              for (int b = 0; b < TN; ++b)
                acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[a][j], bfr[b][j], acc[a][b], 0, 0, 0);
        }
      }
    }
  };

  if constexpr (GL) {
    // ---- main loop: ST-deep LDS-DMA ring, one raw barrier per 128-B k-tile ----
    constexpr int NG = A_SLOTS + B_SLOTS;   // LDS-DMA instructions per thread per k-tile
#pragma unroll
    for (int s0 = 0; s0 < ST - 1; ++s0)
      if (s0 < nkt) load_tile(s0, s0);
    int stage = 0;
    for (int kt = 0; kt < nkt; ++kt) {
      // k-tiles issued after kt (at most ST-2 of them) may stay in flight
      const int ahead = nkt - 1 - kt;
      if (ST >= 4 && ahead >= 2) wait_vmcnt<(ST >= 4 ? 2 * NG : 0)>();
      else if (ST >= 3 && ahead >= 1) wait_vmcnt<(ST >= 3 ? NG : 0)>();
      else wait_vmcnt<0>();
      raw_barrier();                        // k-tile kt visible to all; stage of kt-1 free
      if (kt + ST - 1 < nkt) {
        int ns = stage + ST - 1;
        if (ns >= ST) ns -= ST;
        load_tile(kt + ST - 1, ns);
      }
      compute(stage);
      if (++stage == ST) stage = 0;
    }
    __syncthreads();
  } else {
    // ---- main loop: register-staged double buffer, one barrier per 128-B k-tile ----
    load_tile(0, 0);
    store_tile(0);
    __syncthreads();
    for (int kt = 0; kt < nkt; ++kt) {
      const int cur = kt & 1;
      const bool more = kt + 1 < nkt;
      if (more) load_tile(kt + 1, 0);
      compute(cur);
      if (more) store_tile(cur ^ 1);
      __syncthreads();
    }
  }

  // ---- epilogue: stage the fp32 tile in LDS, then 16-B coalesced row segments ----
  float* st = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int a = 0; a < TM; ++a)
#pragma unroll
    for (int b = 0; b < TN; ++b)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int rl = wm * WTM + a * 32 + (i & 3) + 8 * (i >> 2) + 4 * lh;
        st[rl * EPI_P + wn * WTN + b * 32 + lr] = acc[a][b][i];
      }
  __syncthreads();
  constexpr int CH = BN / 8;              // 8-channel chunks per row
  constexpr int RS = 256 / CH;            // row lanes
  constexpr int NR = BM / RS;             // rows per thread
  const int ch = tid % CH, rr = tid / CH;
  const int col0 = n0 + ch * 8;
  const int nv = p.Ncols - col0;          // valid channels in this chunk (may be <= 0)
  float sc[8], sh[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    sc[i] = 1.0f;
    sh[i] = 0.0f;
    if (EPI == EPI_AFFINE && i < nv) {
      if (p.scale) sc[i] = p.scale[col0 + i];
      if (p.shift) sh[i] = p.shift[col0 + i];
    }
  }
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    const int rl = rr + RS * j;
    int row = m0 + rl;
    float v[8];
    const float4 u0 = *reinterpret_cast<const float4*>(st + rl * EPI_P + ch * 8);
    const float4 u1 = *reinterpret_cast<const float4*>(st + rl * EPI_P + ch * 8 + 4);
    v[0] = u0.x; v[1] = u0.y; v[2] = u0.z; v[3] = u0.w;
    v[4] = u1.x; v[5] = u1.y; v[6] = u1.z; v[7] = u1.w;
    if (row >= M || nv <= 0) continue;
    if (MODE == MODE_DGRAD2) {
      const uint32_t n = fdiv((uint32_t)row, dv_hw);
      const uint32_t rem = (uint32_t)row - n * dv_hw.d;
      const uint32_t ya = fdiv(rem, dv_w);
      const uint32_t xb = rem - ya * dv_w.d;
      row = ((int)n * p.OH + 2 * (int)ya + (cls >> 1)) * p.OWx + 2 * (int)xb + (cls & 1);
    }
    T* dst = reinterpret_cast<T*>(p.dst) + (long)row * p.dst_ld + p.dst_off + col0;
    if (EPI == EPI_AFFINE) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        float a = v[i] * sc[i] + sh[i];
        if (p.act == YMS_ACT_SILU) a = silu_f(a);
        v[i] = a;
      }
      if (p.res) {
        float r[8];
        load8(reinterpret_cast<const T*>(p.res) + (long)row * p.res_ld + p.res_off + col0, nv, r);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] += r[i];
      }
    } else if (EPI == EPI_ACCUM) {
      float r[8];
      load8(dst, nv, r);
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] += r[i];
    }
    store8(dst, nv, v);
  }
  if (EPI == EPI_STATS) {
    // one statistics row per 128-row tile (BM == 128): sum and centred M2 of each column over
    // the valid rows, two passes down the fp32 staging tile (read-only since the barrier above)
    static_assert(EPI != EPI_STATS || BM == 128, "statistics rows are 128 output rows");
    if (tid < BN) {
      const int nrow = min(BM, M - m0);
      float t1 = 0.f, t2 = 0.f;
      for (int r = 0; r < nrow; ++r) t1 += st[r * EPI_P + tid];
      const float mu = t1 / (float)nrow;
      for (int r = 0; r < nrow; ++r) {
        const float d = st[r * EPI_P + tid] - mu;
        t2 += d * d;
      }
      float* so = p.stats + (long)tile_m * 2 * p.stats_ld;
      so[n0 + tid] = t1;
      so[p.stats_ld + n0 + tid] = t2;
      if (tile_n == 0 && tid == 0) p.stats_cnt[tile_m] = (float)nrow;
    }
  }
}

// ------------------------------------------------------------------------------------------
// Persistent NT kernel (16-bit types).  Each block walks output tiles lb, lb+G, lb+2G, ...
// (lb = XCD-remapped block id, G = grid size) as ONE flattened (tile, k-tile) stream: the
// ST-deep LDS-DMA ring keeps prefetching across tile boundaries, so a tile's epilogue overlaps
// the next tile's loads and no pipeline fill/drain is paid per tile.  The epilogue applies
// the affine/SiLU to the fp32 accumulators in registers (BN statistics are reduced from them
// by cross-lane adds), stages the tile as T through the ring stage just consumed, and writes
// 16-B row segments (+ residual / + accumulate in fp32).
// ------------------------------------------------------------------------------------------
constexpr int NTP_MAX_AFFINE_COLS = 512;   // wider affine outputs use conv_nt_kernel
// The kernel body as a function of (parameters, block index, grid size G): conv_ntp_kernel runs it
// with its own launch's (blockIdx.x, gridDim.x), conv_ntp_group_kernel with one member's.
template <typename T, int KS, int MODE, int EPI, int BM, int BN, int WGM, int WGN, int ST, bool UNI>
__device__ __forceinline__ void conv_ntp_body(const NTParams& p, const int bid, const int G) {
  constexpr int NTHR = WGM * WGN * 64;
  constexpr int RPP = NTHR / NT_KCH;                       // rows per load pass (one slot)
  constexpr int SLOT = RPP * 128;                          // LDS bytes per slot
  constexpr int WTM = BM / WGM, WTN = BN / WGN;
  constexpr int TM = WTM / 32, TN = WTN / 32;
  constexpr int A_SLOTS = BM / RPP;
  constexpr bool B_PART = BN < RPP;                         // only the first BN/8 waves load B
  constexpr int B_SLOTS = B_PART ? 1 : BN / RPP;
  constexpr int STAGE = (BM + BN) * 128;
  // statistics: per-wave column partials [WGM][2][BN] + the combiner threads' running moments
  // [3][SROWS*BN] (kept in LDS: three more live VGPRs would cost a block per CU)
  constexpr int RED = (EPI == EPI_STATS) ? (WGM * 2 + 3 * (BM / 128 > 0 ? BM / 128 : 1)) * BN * 4 : 0;
  constexpr int PRM = (EPI == EPI_AFFINE) ? 2 * NTP_MAX_AFFINE_COLS * 4 : 0;
  static_assert((B_PART || BN % RPP == 0) && BM % RPP == 0 && BN <= NTHR, "tile");
  // the output tile is staged through the ring stage just consumed, in NH passes of HR rows
  constexpr int NH = (BM * BN * (int)sizeof(T) > STAGE) ? 2 : 1;
  constexpr int HR = BM / NH;
  static_assert(HR * BN * (int)sizeof(T) <= STAGE && HR % (BM / WGM) == 0, "staging must fit one ring stage");
  // BN statistics: every block walks tiles of ONE column tile (the grid is a multiple of tiles_n),
  // so it keeps per-column running moments of its tiles (Chan merges, in the combiner threads'
  // registers) and writes one row per 128-row half of its tiles, slot lb / tiles_n, at the end
  // (yms_conv_stats_rows = SROWS x grid / tiles_n, counts after the rows)
  constexpr int SROWS = BM / 128 > 0 ? BM / 128 : 1;
  static_assert(BM % 128 == 0 && WGM % SROWS == 0, "statistics rows");
  __shared__ __attribute__((aligned(16))) char smem[ST * STAGE + RED + PRM + 16];
  float* red = reinterpret_cast<float*>(smem + ST * STAGE);
  float* prm = reinterpret_cast<float*>(smem + ST * STAGE + RED);   // [scale | shift] per column

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WGN, wn = wave % WGN;
  const int lr = lane & 31, lh = lane >> 5;
  int M = p.M, nkt = p.nkt, Kc = p.Kc, ntx = 1, cls = 0;
  const char* wp = p.wp;
  FastDiv dv_w = p.div_ow, dv_hw = p.div_ohw;
  if (MODE == MODE_DGRAD2) {
    cls = blockIdx.y;
    M = p.cls_M[cls];
    nkt = p.cls_nkt[cls];
    Kc = p.cls_Kc[cls];
    ntx = p.cls_ntx[cls];
    wp = p.wp + p.cls_woff[cls];
    dv_w = p.cls_div_w[cls];
    dv_hw = p.cls_div_hw[cls];
  }
  const int lb = xcd_remap(bid, G);
  const int ntiles = ((M + BM - 1) / BM) * p.tiles_n;
  if (lb >= ntiles || nkt <= 0) return;
  const int my_tiles = (ntiles - lb + G - 1) / G;
  const int total = my_tiles * nkt;
  if constexpr (EPI == EPI_AFFINE) {
    // per-column BN scale/shift kept in LDS: an epilogue global load would make the compiler
    // drain (vmcnt(0)) the LDS-DMA prefetch of the next tile
    for (int c = tid; c < p.Ncols; c += NTHR) {
      prm[c] = p.scale ? p.scale[c] : 1.0f;
      prm[NTP_MAX_AFFINE_COLS + c] = p.shift ? p.shift[c] : 0.0f;
    }
    __syncthreads();
  }

  // ---- loader (runs ST-1 steps ahead of compute) ----
  // Raw-buffer LDS-DMA (buffer_load_dwordx4 ... lds): a lane whose im2col element lies outside
  // the image (or past K) gets voffset = NT_OOB, beyond the resource's num_records, and the
  // hardware writes zeros into its LDS slot -- no exec-masked branches, no 64-bit address
  // arithmetic.  UNI (cpt % 8 == 0): every lane of a k-tile sits in the same tap, so the tap
  // offset is scalar and each A slot costs one bit test, one add and one select.
  constexpr int NTAPS = MODE == MODE_DGRAD2 ? 4 : KS * KS;
  constexpr int SGN = MODE == MODE_FWD ? 1 : -1;
  constexpr int ES = (int)sizeof(T);
  const __amdgpu_buffer_rsrc_t rs_a =
      __builtin_amdgcn_make_buffer_rsrc((void*)p.src, (short)0, (int)p.src_bytes, NT_RSRC3);
  const __amdgpu_buffer_rsrc_t rs_b = __builtin_amdgcn_make_buffer_rsrc((void*)wp, (short)0, 0x7fffffff, NT_RSRC3);
  auto tap_dyx = [&](int t, int& dy, int& dx) {
    if (MODE == MODE_DGRAD2) {
      dy = ntx == 1 ? t : (t >> 1);
      dx = ntx == 1 ? 0 : (t & 1);
    } else {
      dy = t / KS;
      dx = t - (t / KS) * KS;
    }
  };
  const int q = (tid & 7) ^ ((tid >> 4) & 7), r0 = tid >> 3;   // swizzled source chunk, first row
  const int wv = __builtin_amdgcn_readfirstlane(wave);
  const int tap_row = p.SW * p.src_ld * ES;                    // bytes per source image row
  int a_base[A_SLOTS];                                          // byte offset of tap 0 (+ lane chunk)
  uint32_t a_msk[A_SLOTS];
  uint32_t b_base[B_SLOTS];
  int tap = 0, cc = 0, ld_kt = 0, ld_tile = lb;
  auto setup_rows = [&](int t) {
    const int m0 = (t / p.tiles_n) * BM;
    const int n0 = (t % p.tiles_n) * BN;
#pragma unroll
    for (int i = 0; i < A_SLOTS; ++i) {
      const int m = m0 + r0 + RPP * i;
      const bool row_ok = m < M;
      const uint32_t mm = row_ok ? (uint32_t)m : 0u;
      const uint32_t n = fdiv(mm, dv_hw);
      const uint32_t rem = mm - n * dv_hw.d;
      const uint32_t oy = fdiv(rem, dv_w);
      const uint32_t ox = rem - oy * dv_w.d;
      int y0, x0;
      if (MODE == MODE_FWD) {
        y0 = (int)oy * p.stride - p.pad;
        x0 = (int)ox * p.stride - p.pad;
      } else if (MODE == MODE_DGRAD) {
        y0 = (int)oy + p.pad;
        x0 = (int)ox + p.pad;
      } else {
        y0 = (int)oy + p.cls_c0y[cls];
        x0 = (int)ox + p.cls_c0x[cls];
      }
      a_base[i] = ((((int)n * p.SH + y0) * p.SW + x0) * p.src_ld + p.src_off) * ES + (UNI ? q * 16 : 0);
      uint32_t msk = 0;
#pragma unroll
      for (int tt = 0; tt < NTAPS; ++tt) {
        int dy, dx;
        tap_dyx(tt, dy, dx);
        const int iy = y0 + SGN * dy, ix = x0 + SGN * dx;
        if (row_ok && iy >= 0 && iy < p.SH && ix >= 0 && ix < p.SW) msk |= 1u << tt;
      }
      a_msk[i] = msk;
    }
#pragma unroll
    for (int j = 0; j < B_SLOTS; ++j)
      b_base[j] = (uint32_t)(((n0 + j * RPP + r0) * (nkt * NT_KCH) + q) * 16);
    tap = 0;
    cc = 0;
  };
  setup_rows(ld_tile);
  auto issue = [&](int stage) {
    char* lds_a = smem + stage * STAGE + wv * 1024;
    char* lds_b = smem + stage * STAGE + BM * 128 + wv * 1024;
    if constexpr (UNI) {
      // scalar tap / channel position of this k-tile
      int dy, dx;
      tap_dyx(tap, dy, dx);
      const int delta = SGN * (dy * tap_row + dx * p.src_ld * ES) + cc * 16;
#pragma unroll
      for (int i = 0; i < A_SLOTS; ++i) {
        const uint32_t vo = ((a_msk[i] >> tap) & 1u) ? (uint32_t)(a_base[i] + delta) : NT_OOB;
        blds16(rs_a, lds_a + i * SLOT, vo);
      }
      cc += NT_KCH;
      if (cc >= p.cpt) { cc = 0; ++tap; }
    } else {
      // per-lane K position: kc = kt*8 + q, tap = kc / cpt (exact multiply-shift, host-checked)
      const int kc = ld_kt * NT_KCH + q;
      const int lt = (int)(((uint64_t)(uint32_t)kc * p.cpt_magic) >> 32);
      const int lc = kc - lt * p.cpt;
      int dy, dx;
      if (MODE == MODE_DGRAD2) {
        dy = ntx == 1 ? lt : (lt >> 1);
        dx = ntx == 1 ? 0 : (lt & 1);
      } else if (KS == 3) {
        dy = (lt * 11) >> 5;          // lt / 3 for lt < 9
        dx = lt - 3 * dy;
      } else {
        dy = 0;
        dx = 0;
      }
      const int delta = SGN * (dy * tap_row + dx * p.src_ld * ES) + lc * 16;
      const uint32_t tb = kc < Kc ? (1u << lt) : 0u;
#pragma unroll
      for (int i = 0; i < A_SLOTS; ++i) {
        const uint32_t vo = (a_msk[i] & tb) ? (uint32_t)(a_base[i] + delta) : NT_OOB;
        blds16(rs_a, lds_a + i * SLOT, vo);
      }
    }
    const int kb = ld_kt * (NT_KCH * 16);
    if (!B_PART || wv * 8 < BN) {
#pragma unroll
      for (int j = 0; j < B_SLOTS; ++j)
        blds16(rs_b, lds_b + j * SLOT, b_base[j] + kb);
    }
    if (++ld_kt == nkt) {           // next tile of this block
      ld_kt = 0;
      ld_tile += G;
      if (ld_tile < ntiles) setup_rows(ld_tile);
    }
  };

  // ---- compute ----
  f32x16 acc[TM][TN];
#pragma unroll
  for (int a = 0; a < TM; ++a)
#pragma unroll
    for (int b = 0; b < TN; ++b)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[a][b][i] = 0.0f;
  const int swz = (lr >> 1) & 7;
  auto compute = [&](int stage) {
    const char* A = smem + stage * STAGE;
    const char* B = A + BM * 128;
    u32x4 af[2][TM], bfr[2][TN];
    auto frags = [&](int s, int slot) {
      const int co = ((2 * s + lh) ^ swz) * 16;
#pragma unroll
      for (int a = 0; a < TM; ++a)
        af[slot][a] = *reinterpret_cast<const u32x4*>(A + (wm * WTM + a * 32 + lr) * 128 + co);
#pragma unroll
      for (int b = 0; b < TN; ++b)
        bfr[slot][b] = *reinterpret_cast<const u32x4*>(B + (wn * WTN + b * 32 + lr) * 128 + co);
    };
    frags(0, 0);
#pragma unroll
    for (int s = 0; s < NT_KCH / 2; ++s) {
      if (s + 1 < NT_KCH / 2) frags(s + 1, (s + 1) & 1);
#pragma unroll
      for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b) acc[a][b] = Mfma<T>::mma(af[s & 1][a], bfr[s & 1][b], acc[a][b]);
    }
  };

  // ---- epilogue of one tile (staging through ring stage `stage`) ----
  auto lds_barrier = [&]() {
    __builtin_amdgcn_s_waitcnt((0xF) | (3 << 14) | (0x7 << 4) | (0 << 8));   // lgkmcnt(0) only
    raw_barrier();
  };
  // combiner thread (sr, c) = tid < BN*SROWS owns running-moment slot tid (n, sum, M2)
  float* const run = red + WGM * 2 * BN;
  if constexpr (EPI == EPI_STATS) {
    if (tid < BN * SROWS) {
      run[tid] = 0.f;
      run[BN * SROWS + tid] = 0.f;
      run[2 * BN * SROWS + tid] = 0.f;
    }
  }
  auto epilogue = [&](int t, int stage) {
    const int tile_m = t / p.tiles_n, m0 = tile_m * BM, n0 = (t % p.tiles_n) * BN;
    T* stg = reinterpret_cast<T*>(smem + stage * STAGE);
    // per-column parameters / statistics from the fp32 accumulators
    if constexpr (EPI == EPI_STATS) {
      const int nw = min(WTM, max(0, M - (m0 + wm * WTM)));   // valid rows of this wave
#pragma unroll
      for (int b = 0; b < TN; ++b) {
        float s1, s2;
        wave_col_moments<TM>(acc, b, nw, lh, s1, s2);
        if (lh == 0) {
          red[(wm * 2 + 0) * BN + wn * WTN + b * 32 + lr] = s1;
          red[(wm * 2 + 1) * BN + wn * WTN + b * 32 + lr] = s2;
        }
      }
    }
    if constexpr (EPI == EPI_AFFINE) {
#pragma unroll
      for (int b = 0; b < TN; ++b) {
        const int col = n0 + wn * WTN + b * 32 + lr;
        const bool cv = col < p.Ncols;
        const float sc = cv ? prm[col] : 1.0f;
        const float sh = cv ? prm[NTP_MAX_AFFINE_COLS + col] : 0.0f;
#pragma unroll
        for (int a = 0; a < TM; ++a)
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            float v = acc[a][b][i] * sc + sh;
            if (p.act == YMS_ACT_SILU) v = silu_f(v);
            acc[a][b][i] = v;
          }
      }
    }
    constexpr int CH = BN / 8;      // 16-B chunks per staged row
    constexpr int RS = NTHR / CH;   // rows per pass
    const int ch = tid % CH, rr = tid / CH;
    const int col0 = n0 + ch * 8;
    const int nv = p.Ncols - col0;
#pragma unroll
    for (int h = 0; h < NH; ++h) {
      // h = 0: every wave has finished reading `stage` as MFMA operands; h > 0: every thread
      // has finished reading the previous pass out of the staging rows
      lds_barrier();
      if (NH == 1 || (wm * WTM) / HR == h) {
#pragma unroll
        for (int a = 0; a < TM; ++a)
#pragma unroll
          for (int b = 0; b < TN; ++b)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
              const int rl = wm * WTM - h * HR + a * 32 + (i & 3) + 8 * (i >> 2) + 4 * lh;
              stg[rl * BN + wn * WTN + b * 32 + lr] = (T)acc[a][b][i];
              acc[a][b][i] = 0.0f;
            }
      }
      lds_barrier();
      if constexpr (EPI == EPI_STATS) {
        if (h == 0 && tid < BN * SROWS) {
          const int sr = tid / BN, c = tid - sr * BN;
          constexpr int WPR = WGM / SROWS;    // wave rows per statistics row
          const int r0 = m0 + sr * 128;
          const int nt = min(128, max(0, M - r0));
          if (nt > 0) {
            float t1, t2;
            merge_moments<WPR, WTM>(red + (sr * WPR * 2 + 0) * BN + c, red + (sr * WPR * 2 + 1) * BN + c, 2 * BN,
                                    nt, t1, t2);
            const float rn = run[tid];
            if (rn == 0.f) {
              run[tid] = (float)nt;
              run[BN * SROWS + tid] = t1;
              run[2 * BN * SROWS + tid] = t2;
            } else {
              const float rs = run[BN * SROWS + tid];
              const float nn = rn + (float)nt;
              const float d = t1 / (float)nt - rs / rn;
              run[2 * BN * SROWS + tid] += t2 + d * d * (rn * (float)nt / nn);
              run[BN * SROWS + tid] = rs + t1;
              run[tid] = nn;
            }
          }
        }
      }
#pragma unroll
      for (int j = 0; j < HR / RS; ++j) {
        const int rl = rr + RS * j;
        int row = m0 + h * HR + rl;
        if (row >= M || nv <= 0) continue;
        float v[8];
        unpack8(*reinterpret_cast<const Raw8<T>*>(stg + rl * BN + ch * 8), v);
        if (MODE == MODE_DGRAD2) {
          const uint32_t n = fdiv((uint32_t)row, dv_hw);
          const uint32_t rem = (uint32_t)row - n * dv_hw.d;
          const uint32_t ya = fdiv(rem, dv_w);
          const uint32_t xb = rem - ya * dv_w.d;
          row = ((int)n * p.OH + 2 * (int)ya + (cls >> 1)) * p.OWx + 2 * (int)xb + (cls & 1);
        }
        T* dst = reinterpret_cast<T*>(p.dst) + (long)row * p.dst_ld + p.dst_off + col0;
        if (EPI == EPI_AFFINE && p.res) {
          float r[8];
          load8(reinterpret_cast<const T*>(p.res) + (long)row * p.res_ld + p.res_off + col0, nv, r);
#pragma unroll
          for (int i = 0; i < 8; ++i) v[i] += r[i];
        } else if (EPI == EPI_ACCUM) {
          float r[8];
          load8(dst, nv, r);
#pragma unroll
          for (int i = 0; i < 8; ++i) v[i] += r[i];
        }
        store8(dst, nv, v);
      }
    }
  };

  // ---- flattened (tile, k-tile) stream ----
  constexpr int NG = A_SLOTS + B_SLOTS;
#pragma unroll
  for (int s0 = 0; s0 < ST - 1; ++s0)
    if (s0 < total) issue(s0);
  int stage = 0, ckt = 0, ctile = lb;
  for (int g = 0; g < total; ++g) {
    const int ahead = total - 1 - g;
    // tile g landed; up to ST-2 later tiles stay in flight (counts are per wave: B_PART waves
    // past the B rows issue only the A loads)
    if (!B_PART || wv * 8 < BN) wait_tiles<NG, ST - 2>(ahead);
    else wait_tiles<A_SLOTS, ST - 2>(ahead);
    raw_barrier();
    if (g + ST - 1 < total) {
      int ns = stage + ST - 1;
      if (ns >= ST) ns -= ST;
      issue(ns);
    }
    compute(stage);
    if (++ckt == nkt) {
      epilogue(ctile, stage);
      ckt = 0;
      ctile += G;
    }
    if (++stage == ST) stage = 0;
  }
  if constexpr (EPI == EPI_STATS) {
    if (tid < BN * SROWS) {
      const int sr = tid / BN, c = tid - sr * BN;
      const int row = (lb / p.tiles_n) * SROWS + sr, n0 = (lb % p.tiles_n) * BN;
      float* so = p.stats + (long)row * 2 * p.stats_ld;
      so[n0 + c] = run[BN * SROWS + tid];
      so[p.stats_ld + n0 + c] = run[2 * BN * SROWS + tid];
      if (n0 == 0 && c == 0) p.stats_cnt[row] = run[tid];
    }
  }
}

template <typename T, int KS, int MODE, int EPI, int BM, int BN, int WGM, int WGN, int ST, bool UNI, int OCC = 2>
__global__ __launch_bounds__(WGM * WGN * 64, OCC) void conv_ntp_kernel(NTParams p) {
  conv_ntp_body<T, KS, MODE, EPI, BM, BN, WGM, WGN, ST, UNI>(p, blockIdx.x, gridDim.x);
}

// Up to NT_GROUP_MAX independent convolutions of one template key in ONE launch: member
// blockIdx.z runs exactly its solo launch's decomposition (its own grid size grid[z] as G, so the
// same tile -> block walk and the same statistics slots); gridDim.x is the largest member grid and
// the blocks past a member's own grid leave at once.  (NTGroup is 4 x sizeof(NTParams) + 16 bytes
// of kernel arguments, within the 4 KB limit: static_assert below.)
constexpr int NT_GROUP_MAX = 4;
struct NTGroup {
  NTParams m[NT_GROUP_MAX];
  int grid[NT_GROUP_MAX];
};
static_assert(sizeof(NTGroup) <= 4096, "NTGroup must fit the kernel-argument segment");
template <typename T, int KS, int MODE, int EPI, int BM, int BN, int WGM, int WGN, int ST, bool UNI, int OCC = 2>
__global__ __launch_bounds__(WGM * WGN * 64, OCC) void conv_ntp_group_kernel(NTGroup g) {
  const int z = blockIdx.z;
  const int G = g.grid[z];
  if ((int)blockIdx.x >= G) return;
  conv_ntp_body<T, KS, MODE, EPI, BM, BN, WGM, WGN, ST, UNI>(g.m[z], blockIdx.x, G);
}

// ------------------------------------------------------------------------------------------
// weight packing
// ------------------------------------------------------------------------------------------
template <typename T>
__global__ void pack_weight_kernel(const float* w, T* out, int cout, int cin, int ks, int rows,
                                   int kp_elems, int c8_in, int for_dgrad) {
  // fwd  : out[co][tap*cin8 + ci]   = w[co][ci][tap]        rows = cout_pad
  // dgrad: out[ci][tap*cout8 + co]  = w[co][ci][tap]        rows = cin_pad
  const long total = (long)rows * kp_elems;
  for (long t = blockIdx.x * (long)blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
    const int r = (int)(t / kp_elems);
    const int k = (int)(t % kp_elems);
    const int tap = k / c8_in, c = k % c8_in;
    float v = 0.f;
    if (tap < ks * ks) {
      const int co = for_dgrad ? c : r;
      const int ci = for_dgrad ? r : c;
      if (co < cout && ci < cin) v = w[((long)co * cin + ci) * ks * ks + tap];
    }
    out[t] = (T)v;
  }
}

// All of a plan's weight packs in one launch (training repacks every step): block (x, job)
// handles rows x, x + gridDim.x, ... of job `job`; 32-bit index math only.
__global__ __launch_bounds__(256) void pack_weight_batched_kernel(const yms_pack_job* jobs, char* dst_base) {
  yms_pack_job j = jobs[blockIdx.y];
  j.packed = dst_base + (uintptr_t)j.packed;     // offsets relative to the (per-call) arena base
  const int kk = j.ks * j.ks;
  for (int r = blockIdx.x; r < j.rows; r += gridDim.x) {
    for (int k = threadIdx.x; k < j.kp_elems; k += 256) {
      const int tap = k / j.c8_in, c = k - tap * j.c8_in;
      float v = 0.f;
      if (tap < kk) {
        const int co = j.for_dgrad ? c : r;
        const int ci = j.for_dgrad ? r : c;
        if (co < j.cout && ci < j.cin) {
          const bool hi = j.w2 && co >= j.split;
          v = (hi ? j.w2 : j.w)[((long)(hi ? co - j.split : co) * j.cin + ci) * kk + tap];
        }
      }
      const long o = (long)r * j.kp_elems + k;
      if (j.dtype == YMS_BF16) reinterpret_cast<bf16*>(j.packed)[o] = (bf16)v;
      else if (j.dtype == YMS_F16) reinterpret_cast<f16*>(j.packed)[o] = (f16)v;
      else reinterpret_cast<float*>(j.packed)[o] = v;
    }
  }
}

// stride-2 dgrad: 4 parity-class blocks, block c = [cin_pad128][kp_c]; K = (jy, jx, co8)
struct Dg2Pack {
  long off[4];       // element offset of each class block
  int kp[4];         // elements per row of each class block
  int ntx[4], kh0[4], kw0[4];
};
template <typename T>
__global__ void pack_weight_dgrad2_kernel(const float* w, T* out, int cout, int cin, int ks, int rows, int c8,
                                          Dg2Pack g, long total) {
  for (long t = blockIdx.x * (long)blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
    int c = 0;
    while (c < 3 && t >= g.off[c + 1]) ++c;
    const long e = t - g.off[c];
    const int r = (int)(e / g.kp[c]);       // ci
    const int k = (int)(e % g.kp[c]);
    const int tl = k / c8, co = k % c8;
    const int jy = tl / g.ntx[c], jx = tl % g.ntx[c];
    const int kh = g.kh0[c] + 2 * jy, kw = g.kw0[c] + 2 * jx;
    float v = 0.f;
    if (kh < ks && kw < ks && co < cout && r < cin) v = w[((long)co * cin + r) * ks * ks + kh * ks + kw];
    out[t] = (T)v;
  }
  (void)rows;
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
struct PackGeo {
  int rows, c8_in, cpt, kc, nkt, kp_elems;
};
static PackGeo pack_geo(const yms_conv_shape* s, int for_dgrad) {
  PackGeo g;
  const int es = elem_size(s->dtype);
  const int cin_k = for_dgrad ? s->cout : s->cin;    // channels along K
  const int cout_r = for_dgrad ? s->cin : s->cout;   // rows
  g.c8_in = (int)rup(cin_k, 8);
  g.cpt = g.c8_in * es / 16;
  g.kc = s->k * s->k * g.cpt;
  g.nkt = cdiv(g.kc, NT_KCH);
  g.kp_elems = g.nkt * NT_KCH * 16 / es;
  g.rows = (int)rup(cout_r, 128);
  return g;
}

struct Dg2Geo {
  int M[4], nkt[4], Kc[4], ntx[4], nty[4], c0y[4], c0x[4], kh0[4], kw0[4], Ha[4], Wa[4], kp[4];
  long off_elems[5];
  int rows, cpt;
};
static Dg2Geo dg2_geo(const yms_conv_shape* s) {
  Dg2Geo g;
  const int es = elem_size(s->dtype);
  const int c8 = (int)rup(s->cout, 8);
  g.cpt = c8 * es / 16;
  g.rows = (int)rup(s->cin, 128);
  g.off_elems[0] = 0;
  for (int c = 0; c < 4; ++c) {
    const int ry = c >> 1, rx = c & 1;
    const int kh0 = (ry + s->pad) & 1, kw0 = (rx + s->pad) & 1;
    g.kh0[c] = kh0;
    g.kw0[c] = kw0;
    g.nty[c] = (s->k - kh0 + 1) / 2;
    g.ntx[c] = (s->k - kw0 + 1) / 2;
    g.c0y[c] = (ry + s->pad - kh0) / 2;
    g.c0x[c] = (rx + s->pad - kw0) / 2;
    g.Ha[c] = (s->h - ry + 1) / 2;
    g.Wa[c] = (s->w - rx + 1) / 2;
    g.M[c] = s->n * g.Ha[c] * g.Wa[c];
    g.Kc[c] = g.nty[c] * g.ntx[c] * g.cpt;
    g.nkt[c] = std::max(1, cdiv(g.Kc[c], NT_KCH));
    g.kp[c] = g.nkt[c] * NT_KCH * 16 / es;
    g.off_elems[c + 1] = g.off_elems[c] + (long)g.rows * g.kp[c];
  }
  return g;
}

struct TileChoice { int cfg, bn; };
static TileChoice choose_tile(int ncols) {
  // One column tile whenever N <= 128: every extra column tile re-reads the whole im2col
  // A operand, which costs more than the padded MFMA columns at these sizes.
  if (ncols <= 32) return TileChoice{2, 32};
  if (ncols <= 64) return TileChoice{1, 64};
  if (ncols <= 128) return TileChoice{0, 128};
  // wider: 128-column tiles unless that pads by more than 25%
  const long p128 = rup(ncols, 128), p64 = rup(ncols, 64);
  if (p128 * 4 > ncols * 5 && p64 < p128) return TileChoice{1, 64};
  return TileChoice{0, 128};
}

// The ONE route decision of a forward (dgrad = 0) or input gradient (dgrad = 1) with epilogue epi: the
// solo entry points, launch_nt and the grouped calls all read it.
struct ConvRoute {
  enum Kind {
    DIRECT,              // small-channel 3x3: conv_direct_kernel (conv_direct.hip), geometry dg
    NT,                  // conv_nt_kernel: fp32, and 16-bit affine outputs wider than NTP_MAX_AFFINE_COLS
    NTP                  // persistent 16-bit conv_ntp_kernel, with the UNI loader when uni
  } kind;
  bool parity;           // stride-2 input gradient: the four output parity classes (MODE_DGRAD2)
  int cfg;               // tile config of NT / NTP (choose_tile)
  bool uni;
  DirectGeo dg;
  PackGeo pg;            // the GEMM's K geometry (conv_params reads it), or the parity classes' d2
  Dg2Geo d2;
  // the grouped kernel serves the persistent stride-1 GEMM in its two wide tile configs (the 32-column
  // one no grouped caller has needed)
  bool groupable() const { return kind == NTP && !parity && (cfg == 0 || cfg == 1); }
};
static ConvRoute conv_route(const yms_conv_shape* s, int dgrad, int epi) {
  ConvRoute r{};
  if (conv_direct_geometry(s, dgrad, &r.dg)) return r;
  const int ncols = dgrad ? s->cin : s->cout;
  r.parity = dgrad && s->stride == 2;
  r.cfg = choose_tile(ncols).cfg;
  r.kind = s->dtype == YMS_F32 || (epi == EPI_AFFINE && ncols > NTP_MAX_AFFINE_COLS) ? ConvRoute::NT : ConvRoute::NTP;
  if (r.parity) r.d2 = dg2_geo(s);
  else r.pg = pack_geo(s, dgrad);
  r.uni = (r.parity ? r.d2.cpt : r.pg.cpt) % NT_KCH == 0;
  return r;
}

static int cu_count() { return conv_cu_count(); }

// forward: statistics (training) grids persistent at 1x (the side-stream wgrads hold CUs: 4x
// measured 19.43 -> 19.9 ms/step); eval grids 4x (finer work units balance around the
// overlapped NMS of the serving pipeline: 2.65 -> 2.58 ms/batch).  (Round 4, measured and dropped:
// 256-row tiles of 16 waves at 1 block per CU.)
static int nt_fwd_mult(bool stats) { return stats ? 1 : 4; }
// dgrad grids: one block per output tile (no persistent cap)
constexpr int NT_DGRAD_MULT = 1 << 16;

struct NtpGeo { int bm, bn, occ; };
static NtpGeo ntp_geo(int cfg) {
  if (cfg == 0) return NtpGeo{128, 128, 2};
  if (cfg == 1) return NtpGeo{128, 64, 3};
  return NtpGeo{256, 32, 2};
}

// persistent grid: OCC resident blocks per CU (x mult), at most one block per tile.  Statistics
// launches round it down to a multiple of tiles_n, so every block walks tiles of one column tile
// (conv_ntp_kernel's per-block statistics slots).
static long ntp_grid(long M, int tiles_n, int bm, long occ_blocks_per_cu, bool stats) {
  const long ntiles = (long)cdiv(M, bm) * tiles_n;
  long g = std::max<long>(1, std::min<long>(ntiles, occ_blocks_per_cu * cu_count()));
  if (stats) g = std::max<long>(tiles_n, g - g % tiles_n);
  return g;
}

// p.M is the largest parity class for DGRAD2
template <typename K>
static void launch_persistent(K kernel, const NTParams& p, int bm, unsigned gy, hipStream_t st, long occ, int nthr,
                              bool stats) {
  const unsigned gx = (unsigned)ntp_grid(p.M, p.tiles_n, bm, occ, stats);
  hipLaunchKernelGGL(kernel, dim3(gx, gy), dim3(nthr), 0, st, p);
}

template <typename T, int KS, int MODE, int EPI, bool UNI>
static void launch_ntp(const NTParams& p0, int cfg, unsigned gy, hipStream_t st) {
  NTParams p = p0;
  // dgrad grids: one block per output tile by default.  The weight gradients run beside dgrad on
  // the side stream, and persistent blocks that start late on CUs the wgrad kernels hold would
  // each still owe their fixed share of tiles (interleaved A/B: 19.91 -> 19.74 ms/step).
  const bool stats = EPI == EPI_STATS;
  const long mult = MODE == MODE_FWD ? nt_fwd_mult(stats) : NT_DGRAD_MULT;
  const NtpGeo g = ntp_geo(cfg);
  p.tiles_n = cdiv(p.Ncols, g.bn);
  // 8-wave blocks at 2-3 per CU (4-6 waves per SIMD) hide the ds_read -> MFMA and barrier
  // latencies that 4-wave blocks expose
  // (round 4, measured and dropped: 256 x 128 tiles of 8 waves with 64 x 64 wave tiles, 5-40 %
  // slower, and 128 x 128 tiles of 4 such waves, within +-5 %: profiles/r04b_conv_micro_v*.txt)
  if (cfg == 0) {
    launch_persistent(conv_ntp_kernel<T, KS, MODE, EPI, 128, 128, 2, 4, 2, UNI, 2>, p, 128, gy, st, g.occ * mult, 512, stats);
  } else if (cfg == 1) {
    launch_persistent(conv_ntp_kernel<T, KS, MODE, EPI, 128, 64, 4, 2, 2, UNI, 3>, p, 128, gy, st, g.occ * mult, 512, stats);
  } else {
    launch_persistent(conv_ntp_kernel<T, KS, MODE, EPI, 256, 32, 8, 1, 2, UNI, 2>, p, 256, gy, st, g.occ * mult, 512, stats);
  }
}

template <typename T, int KS, int MODE, int EPI>
static void launch_nt(const NTParams& p0, const ConvRoute& r, hipStream_t st) {
  NTParams p = p0;
  const int cfg = r.cfg;
  const unsigned gy = MODE == MODE_DGRAD2 ? 4u : 1u;
  if constexpr (sizeof(T) == 2) {
    if (r.kind == ConvRoute::NTP) {
      if (r.uni) launch_ntp<T, KS, MODE, EPI, true>(p, cfg, gy, st);
      else launch_ntp<T, KS, MODE, EPI, false>(p, cfg, gy, st);
      return;
    }
  }
  if (cfg == 0) {
    p.tiles_n = cdiv(p.Ncols, 128);
    dim3 grid((unsigned)(cdiv(p.M, 128) * p.tiles_n), gy);
    hipLaunchKernelGGL((conv_nt_kernel<T, KS, MODE, EPI, 128, 128, 2, 2, 2>), grid, dim3(256), 0, st, p);
  } else if (cfg == 1) {
    p.tiles_n = cdiv(p.Ncols, 64);
    dim3 grid((unsigned)(cdiv(p.M, 128) * p.tiles_n), gy);
    hipLaunchKernelGGL((conv_nt_kernel<T, KS, MODE, EPI, 128, 64, 2, 2, 3>), grid, dim3(256), 0, st, p);
  } else {
    p.tiles_n = cdiv(p.Ncols, 32);
    dim3 grid((unsigned)(cdiv(p.M, 128) * p.tiles_n), gy);
    hipLaunchKernelGGL((conv_nt_kernel<T, KS, MODE, EPI, 128, 32, 4, 1, 3>), grid, dim3(256), 0, st, p);
  }
}

// raw-buffer source extent and the exact kc / cpt multiply-shift for the 16-bit loader
static bool set_src_geometry(NTParams& p, long n, long h, long w, long ld, int es, int max_kc) {
  const long bytes = n * h * w * ld * es;
  if (es == 2 && bytes >= (1l << 31) - (1l << 20)) return false;
  p.src_bytes = (uint32_t)std::min<long>(bytes, 0x7fffffffl);
  p.cpt_magic = ((1ull << 32) + (uint64_t)p.cpt - 1) / (uint64_t)p.cpt;
  for (int kc = 0; kc < max_kc; ++kc)
    if ((int)(((uint64_t)(uint32_t)kc * p.cpt_magic) >> 32) != kc / p.cpt) return false;
  return true;
}

// the NT loader addresses its source with 32-bit element offsets
static bool offsets32(long n, long h, long w, long ld) { return n * h * w * ld < (1l << 31) - (1l << 20); }

template <int MODE, int EPI>
static yms_status dispatch_nt(const NTParams& p, int dtype, int ks, const ConvRoute& r, hipStream_t st) {
#define YMS_NT_CASE(T)                                          \
  if constexpr (MODE == MODE_DGRAD2) launch_nt<T, 3, MODE, EPI>(p, r, st);   \
  else if (ks == 1) launch_nt<T, 1, MODE, EPI>(p, r, st);     \
  else launch_nt<T, 3, MODE, EPI>(p, r, st);
  if (dtype == YMS_BF16) { YMS_NT_CASE(bf16) }
  else if (dtype == YMS_F16) { YMS_NT_CASE(f16) }
  else { YMS_NT_CASE(float) }
#undef YMS_NT_CASE
  return launch_status();
}


}  // namespace yms

// yms_cu_count_set's override (0 = none) sits in front of the cached device value: every geometry
// decision calls conv_cu_count() at call time and no memo is keyed on it.
static int cu_override = 0;

int yms::conv_cu_count() {
  if (cu_override > 0) return cu_override;
  static int n = 0;
  if (n == 0) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
      n = 256;
  }
  return n;
}

extern "C" int yms_cu_count_set(int n) {
  const int prev = cu_override;
  if (n >= 0) cu_override = n;
  return prev;
}

using namespace yms;

extern "C" {

size_t yms_conv_packed_elems(const yms_conv_shape* s, int for_dgrad) {
  if (!shape_ok(s)) return 0;
  if (for_dgrad && s->stride == 2) return (size_t)dg2_geo(s).off_elems[4];
  PackGeo g = pack_geo(s, for_dgrad);
  return (size_t)g.rows * g.kp_elems;
}

yms_status yms_pack_job_init(const yms_conv_shape* s, const float* w, void* packed, int for_dgrad,
                             yms_pack_job* job) {
  if (!shape_ok(s) || !w || !job) return YMS_ERR_INVALID;   // packed may be an offset (0 allowed)
  if (for_dgrad && s->stride == 2) return YMS_ERR_UNSUPPORTED;   // parity-class packing: yms_conv_pack_weight
  PackGeo g = pack_geo(s, for_dgrad);
  job->w = w;
  job->packed = packed;
  job->cout = s->cout;
  job->cin = s->cin;
  job->ks = s->k;
  job->rows = g.rows;
  job->kp_elems = g.kp_elems;
  job->c8_in = g.c8_in;
  job->for_dgrad = for_dgrad;
  job->dtype = s->dtype;
  job->w2 = nullptr;
  job->split = 0;
  return YMS_OK;
}

yms_status yms_conv_pack_weights_batched(int njobs, const yms_pack_job* jobs_dev, void* dst_base, void* stream) {
  if (njobs < 0 || (njobs > 0 && !jobs_dev)) return YMS_ERR_INVALID;
  if (njobs == 0) return YMS_OK;
  if (njobs > 65535) return YMS_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(pack_weight_batched_kernel, dim3(64, (unsigned)njobs), dim3(256), 0, (hipStream_t)stream,
                     jobs_dev, (char*)dst_base);
  return launch_status();
}

yms_status yms_conv_pack_weight(const yms_conv_shape* s, const float* w, void* packed,
                                int for_dgrad, void* stream) {
  if (!shape_ok(s) || !w || !packed) return YMS_ERR_INVALID;
  hipStream_t st = (hipStream_t)stream;
  if (for_dgrad && s->stride == 2) {
    Dg2Geo d = dg2_geo(s);
    Dg2Pack pk;
    for (int c = 0; c < 4; ++c) {
      pk.off[c] = d.off_elems[c];
      pk.kp[c] = d.kp[c];
      pk.ntx[c] = d.ntx[c];
      pk.kh0[c] = d.kh0[c];
      pk.kw0[c] = d.kw0[c];
    }
    const long total = d.off_elems[4];
    const int c8 = (int)rup(s->cout, 8);
    dim3 grid((unsigned)std::min<long>(cdiv(total, 256), 4096));
    if (s->dtype == YMS_BF16)
      hipLaunchKernelGGL(pack_weight_dgrad2_kernel<bf16>, grid, dim3(256), 0, st, w, (bf16*)packed, s->cout, s->cin, s->k, d.rows, c8, pk, total);
    else if (s->dtype == YMS_F16)
      hipLaunchKernelGGL(pack_weight_dgrad2_kernel<f16>, grid, dim3(256), 0, st, w, (f16*)packed, s->cout, s->cin, s->k, d.rows, c8, pk, total);
    else
      hipLaunchKernelGGL(pack_weight_dgrad2_kernel<float>, grid, dim3(256), 0, st, w, (float*)packed, s->cout, s->cin, s->k, d.rows, c8, pk, total);
    return launch_status();
  }
  PackGeo g = pack_geo(s, for_dgrad);
  const long total = (long)g.rows * g.kp_elems;
  dim3 grid((unsigned)std::min<long>(cdiv(total, 256), 4096));
  if (s->dtype == YMS_BF16)
    hipLaunchKernelGGL(pack_weight_kernel<bf16>, grid, dim3(256), 0, st, w, (bf16*)packed, s->cout, s->cin, s->k, g.rows, g.kp_elems, g.c8_in, for_dgrad);
  else if (s->dtype == YMS_F16)
    hipLaunchKernelGGL(pack_weight_kernel<f16>, grid, dim3(256), 0, st, w, (f16*)packed, s->cout, s->cin, s->k, g.rows, g.kp_elems, g.c8_in, for_dgrad);
  else
    hipLaunchKernelGGL(pack_weight_kernel<float>, grid, dim3(256), 0, st, w, (float*)packed, s->cout, s->cin, s->k, g.rows, g.kp_elems, g.c8_in, for_dgrad);
  return launch_status();
}

int yms_conv_stats_rows(const yms_conv_shape* s) {
  if (!shape_ok(s)) return 0;
  DirectGeo dg;
  if (conv_direct_geometry(s, 0, &dg)) return dg.grid;   // conv_direct_kernel: one row per block
  const long M = (long)s->n * s->ho * s->wo;
  if (s->dtype == YMS_F32) return (int)cdiv(M, 128);     // conv_nt_kernel: one row per 128-row tile
  const NtpGeo g = ntp_geo(choose_tile(s->cout).cfg);    // conv_ntp_kernel: one slot per block
  const int tiles_n = cdiv(s->cout, g.bn);
  return (int)(ntp_grid(M, tiles_n, g.bm, (long)g.occ * nt_fwd_mult(true), true) / tiles_n) * (g.bm / 128);
}
int yms_conv_stats_ld(const yms_conv_shape* s) {
  if (!shape_ok(s)) return 0;
  return (int)rup(s->cout, 128);
}

}  // extern "C"

// The implicit-GEMM forward's kernel parameters (everything but tiles_n, which the launch sets from
// its tile shape): shared by the solo and the grouped forward.
static yms_status conv_params(const yms_conv_fwd_job& j, const ConvRoute& r, NTParams& p) {
  const yms_conv_shape* s = &j.shape;
  const int es = elem_size(s->dtype);
  const PackGeo& g = r.pg;
  p = NTParams{};
  p.src = (const char*)j.x;
  p.wp = (const char*)j.wpacked;
  p.dst = (char*)j.y;
  p.src_ld = j.x_ld; p.src_off = j.x_off; p.dst_ld = j.y_ld; p.dst_off = j.y_off;
  p.scale = j.scale; p.shift = j.shift; p.act = j.act;
  p.res = (const char*)j.res; p.res_ld = j.res_ld; p.res_off = j.res_off;
  p.stats = j.stats;
  p.stats_ld = (int)rup(s->cout, 128);
  if (j.stats) p.stats_cnt = j.stats + (long)yms_conv_stats_rows(s) * 2 * p.stats_ld;
  p.SH = s->h; p.SW = s->w; p.OW = s->wo;
  if (!offsets32(s->n, s->h, s->w, j.x_ld)) return YMS_ERR_UNSUPPORTED;
  p.stride = s->stride; p.pad = s->pad;
  p.cpt = g.cpt; p.Kc = g.kc; p.nkt = g.nkt;
  if (!set_src_geometry(p, s->n, s->h, s->w, j.x_ld, es, g.nkt * NT_KCH)) return YMS_ERR_UNSUPPORTED;
  p.M = s->n * s->ho * s->wo;
  p.Ncols = s->cout;
  p.div_ow = make_fastdiv(s->wo);
  p.div_ohw = make_fastdiv(s->ho * s->wo);
  return YMS_OK;
}

static bool args_ok(const yms_conv_fwd_job& j) {
  const yms_conv_shape* s = &j.shape;
  if (!shape_ok(s) || !j.x || !j.wpacked || !j.y) return false;
  if (!view_ok(j.x_ld, j.x_off, s->cin) || !view_ok(j.y_ld, j.y_off, s->cout)) return false;
  return !j.res || view_ok(j.res_ld, j.res_off, s->cout);
}
static int epi_of(const yms_conv_fwd_job& j) { return j.stats ? EPI_STATS : EPI_AFFINE; }
static ConvRoute route_of(const yms_conv_fwd_job& j) { return conv_route(&j.shape, 0, epi_of(j)); }

// One forward (arguments checked), solo: yms_conv_fwd, and the grouped call's jobs that no group takes.
static yms_status conv_solo(const yms_conv_fwd_job& j, const ConvRoute& r, hipStream_t st) {
  const yms_conv_shape* s = &j.shape;
  if (r.kind == ConvRoute::DIRECT)          // statistics included
    return conv_direct_launch(s, 0, r.dg, j.x, j.x_ld, j.x_off, j.wpacked, j.y, j.y_ld, j.y_off, j.scale, j.shift,
                              j.act, j.res, j.res_ld, j.res_off, j.stats, 0, st);
  NTParams p;
  if (yms_status e = conv_params(j, r, p)) return e;
  if (j.stats) return dispatch_nt<MODE_FWD, EPI_STATS>(p, s->dtype, s->k, r, st);
  return dispatch_nt<MODE_FWD, EPI_AFFINE>(p, s->dtype, s->k, r, st);
}

static bool args_ok(const yms_conv_dgrad_job& j) {
  const yms_conv_shape* s = &j.shape;
  if (!shape_ok(s) || !j.dz || !j.wpacked_t || !j.dx) return false;
  return view_ok(j.dz_ld, j.dz_off, s->cout) && view_ok(j.dx_ld, j.dx_off, s->cin);
}
static int epi_of(const yms_conv_dgrad_job& j) { return j.accumulate ? EPI_ACCUM : EPI_STORE; }
static ConvRoute route_of(const yms_conv_dgrad_job& j) { return conv_route(&j.shape, 1, epi_of(j)); }

// The input gradient's kernel parameters: those common to both strides, then the stride-1 GEMM's or the
// parity classes' geometry (YMS_ERR_UNSUPPORTED: extent).  p.M == 0: nothing to launch.
static yms_status conv_params(const yms_conv_dgrad_job& j, const ConvRoute& r, NTParams& p) {
  const yms_conv_shape* s = &j.shape;
  const int es = elem_size(s->dtype);
  p = NTParams{};
  p.src = (const char*)j.dz;
  p.wp = (const char*)j.wpacked_t;
  p.dst = (char*)j.dx;
  p.src_ld = j.dz_ld; p.src_off = j.dz_off; p.dst_ld = j.dx_ld; p.dst_off = j.dx_off;
  p.SH = s->ho; p.SW = s->wo; p.OW = s->w;
  p.stride = s->stride; p.pad = s->pad;
  p.Ncols = s->cin;
  p.OH = s->h; p.OWx = s->w;
  if (!offsets32(s->n, s->ho, s->wo, j.dz_ld)) return YMS_ERR_UNSUPPORTED;
  if (!r.parity) {
    const PackGeo& g = r.pg;
    p.cpt = g.cpt; p.Kc = g.kc; p.nkt = g.nkt;
    if (!set_src_geometry(p, s->n, s->ho, s->wo, j.dz_ld, es, g.nkt * NT_KCH)) return YMS_ERR_UNSUPPORTED;
    p.M = s->n * s->h * s->w;
    p.div_ow = make_fastdiv(s->w);
    p.div_ohw = make_fastdiv(s->h * s->w);
    return YMS_OK;
  }
  const Dg2Geo& d = r.d2;
  p.cpt = d.cpt;
  if (!set_src_geometry(p, s->n, s->ho, s->wo, j.dz_ld, es, *std::max_element(d.nkt, d.nkt + 4) * NT_KCH))
    return YMS_ERR_UNSUPPORTED;
  p.M = 0;
  for (int c = 0; c < 4; ++c) {
    p.cls_M[c] = d.M[c];
    p.cls_nkt[c] = d.nkt[c];
    p.cls_Kc[c] = d.Kc[c];
    p.cls_ntx[c] = d.ntx[c];
    p.cls_c0y[c] = d.c0y[c];
    p.cls_c0x[c] = d.c0x[c];
    p.cls_woff[c] = d.off_elems[c] * es;
    p.cls_div_w[c] = make_fastdiv(std::max(1, d.Wa[c]));
    p.cls_div_hw[c] = make_fastdiv(std::max(1, d.Ha[c] * d.Wa[c]));
    p.M = std::max(p.M, d.M[c]);
  }
  return YMS_OK;
}

// One input gradient (arguments checked), solo.
static yms_status conv_solo(const yms_conv_dgrad_job& j, const ConvRoute& r, hipStream_t st) {
  const yms_conv_shape* s = &j.shape;
  if (r.kind == ConvRoute::DIRECT)
    return conv_direct_launch(s, 1, r.dg, j.dz, j.dz_ld, j.dz_off, j.wpacked_t, j.dx, j.dx_ld, j.dx_off, nullptr,
                              nullptr, 0, nullptr, 0, 0, nullptr, j.accumulate, st);
  NTParams p;
  if (yms_status e = conv_params(j, r, p)) return e;
  if (r.parity) {
    if (p.M == 0) return YMS_OK;
    if (j.accumulate) return dispatch_nt<MODE_DGRAD2, EPI_ACCUM>(p, s->dtype, s->k, r, st);
    return dispatch_nt<MODE_DGRAD2, EPI_STORE>(p, s->dtype, s->k, r, st);
  }
  if (j.accumulate) return dispatch_nt<MODE_DGRAD, EPI_ACCUM>(p, s->dtype, s->k, r, st);
  return dispatch_nt<MODE_DGRAD, EPI_STORE>(p, s->dtype, s->k, r, st);
}

// One job of a grouped call: key < 0 runs through the solo entry point.
struct GroupMember {
  int job, key = -1;
  ConvRoute r;
  NTParams p;
};
static int group_key(const yms_conv_shape& s, int epi, const ConvRoute& r) {
  return (((s.dtype * 4 + s.k) * 8 + epi) * 4 + r.cfg) * 2 + (r.uni ? 1 : 0);
}

// Mirrors launch_ntp for n members of one key: each member's tiles_n and grid as its solo launch.
template <typename T, int KS, int MODE, int EPI, bool UNI>
static void launch_ntp_group(const GroupMember* const* ms, int n, int cfg, hipStream_t st) {
  const bool stats = EPI == EPI_STATS;
  const long mult = MODE == MODE_FWD ? nt_fwd_mult(stats) : NT_DGRAD_MULT;
  const NtpGeo g = ntp_geo(cfg);
  NTGroup grp{};
  unsigned gx = 1;
  for (int i = 0; i < n; ++i) {
    grp.m[i] = ms[i]->p;
    grp.m[i].tiles_n = cdiv(grp.m[i].Ncols, g.bn);
    grp.grid[i] = (int)ntp_grid(grp.m[i].M, grp.m[i].tiles_n, g.bm, g.occ * mult, stats);
    gx = std::max(gx, (unsigned)grp.grid[i]);
  }
  // (forward grids are persistent, so the members' grids are close; input-gradient grids are one
  // block per tile, so a small member's z-slice is mostly blocks that leave at once -- at B = 64 about
  // 2400 of 3200 for the 40^2 level and 3000 for the 20^2 one: a dispatch cost of a few microseconds)
  const dim3 grid(gx, 1, (unsigned)n);
  if (cfg == 0)
    hipLaunchKernelGGL((conv_ntp_group_kernel<T, KS, MODE, EPI, 128, 128, 2, 4, 2, UNI, 2>), grid, dim3(512), 0, st, grp);
  else
    hipLaunchKernelGGL((conv_ntp_group_kernel<T, KS, MODE, EPI, 128, 64, 4, 2, 2, UNI, 3>), grid, dim3(512), 0, st, grp);
}

template <int MODE, int EPI>
static void dispatch_group_epi(const GroupMember* const* ms, int n, hipStream_t st) {
  const int key = ms[0]->key;
  const bool uni = key & 1;
  const int cfg = (key >> 1) & 3, ks = (key >> 6) & 3, dtype = key >> 8;
#define YMS_GRP_CASE(T)                                                                  \
  if (ks == 1) {                                                                         \
    if (uni) launch_ntp_group<T, 1, MODE, EPI, true>(ms, n, cfg, st);                    \
    else launch_ntp_group<T, 1, MODE, EPI, false>(ms, n, cfg, st);                       \
  } else {                                                                               \
    if (uni) launch_ntp_group<T, 3, MODE, EPI, true>(ms, n, cfg, st);                    \
    else launch_ntp_group<T, 3, MODE, EPI, false>(ms, n, cfg, st);                       \
  }
  if (dtype == YMS_BF16) { YMS_GRP_CASE(bf16) }
  else { YMS_GRP_CASE(f16) }
#undef YMS_GRP_CASE
}

// Launches the members key by key (first appearance order), then the solo jobs in job order.
// count != nullptr: launches nothing and counts the calls it would make (grouped launches + solo calls).
template <int MODE, typename Solo>
static yms_status launch_groups(const std::vector<GroupMember>& ms, hipStream_t st, Solo solo, int* count = nullptr) {
  std::vector<char> done(ms.size(), 0);
  std::vector<int> singles;
  for (size_t i = 0; i < ms.size(); ++i) {
    if (done[i]) continue;
    if (ms[i].key < 0) { singles.push_back(ms[i].job); continue; }
    const GroupMember* same[NT_GROUP_MAX];
    int n = 0;
    size_t j = i;
    for (; j < ms.size() && n < NT_GROUP_MAX; ++j)
      if (!done[j] && ms[j].key == ms[i].key) { same[n++] = &ms[j]; done[j] = 1; }
    if (n == 1) { singles.push_back(ms[i].job); continue; }
    if (count) { ++*count; continue; }
    const int epi = (ms[i].key >> 3) & 7;
    if (MODE == MODE_FWD) {
      if (epi == EPI_STATS) dispatch_group_epi<MODE_FWD, EPI_STATS>(same, n, st);
      else dispatch_group_epi<MODE_FWD, EPI_AFFINE>(same, n, st);
    } else {
      if (epi == EPI_ACCUM) dispatch_group_epi<MODE_DGRAD, EPI_ACCUM>(same, n, st);
      else dispatch_group_epi<MODE_DGRAD, EPI_STORE>(same, n, st);
    }
    if (yms_status e = launch_status()) return e;
  }
  std::sort(singles.begin(), singles.end());
  if (count) { *count += (int)singles.size(); return YMS_OK; }
  for (int i : singles)
    if (yms_status e = solo(i)) return e;
  return YMS_OK;
}

// ---- grouped launches -----------------------------------------------------------------------
// The jobs of one call are partitioned by kernel template key (dtype, k, epilogue, tile config,
// UNI loader); each key's members go out NT_GROUP_MAX at a time as one conv_ntp_group_kernel launch.
// A job alone in its key, and every job whose route is not groupable (ConvRoute: the direct 3x3
// route, fp32, the stride-2 input gradient, affine outputs wider than NTP_MAX_AFFINE_COLS, the
// 32-column tile config), runs as its solo call, in job order.
template <int MODE, typename Job>
static yms_status conv_group(int njobs, const Job* jobs, void* stream, int* count) {
  if (njobs < 0 || (njobs > 0 && !jobs)) return YMS_ERR_INVALID;
  std::vector<GroupMember> ms;
  for (int i = 0; i < njobs; ++i) {
    if (!args_ok(jobs[i])) return YMS_ERR_INVALID;
    GroupMember m{};
    m.job = i;
    m.r = route_of(jobs[i]);
    if (m.r.groupable()) {
      if (yms_status e = conv_params(jobs[i], m.r, m.p)) return e;
      m.key = group_key(jobs[i].shape, epi_of(jobs[i]), m.r);
    }
    ms.push_back(m);
  }
  return launch_groups<MODE>(ms, (hipStream_t)stream,
                             [&](int i) { return conv_solo(jobs[i], ms[i].r, (hipStream_t)stream); }, count);
}

extern "C" {

yms_status yms_conv_fwd(const yms_conv_shape* s, const void* x, int x_ld, int x_off,
                        const void* wpacked, void* y, int y_ld, int y_off,
                        const float* scale, const float* shift, int act,
                        const void* res, int res_ld, int res_off, float* stats, void* stream) {
  if (!s) return YMS_ERR_INVALID;
  const yms_conv_fwd_job j{*s, x, x_ld, x_off, wpacked, y, y_ld, y_off, scale, shift, act, res, res_ld, res_off, stats};
  return args_ok(j) ? conv_solo(j, route_of(j), (hipStream_t)stream) : YMS_ERR_INVALID;
}

yms_status yms_conv_dgrad(const yms_conv_shape* s, const void* dz, int dz_ld, int dz_off,
                          const void* wpacked_t, void* dx, int dx_ld, int dx_off,
                          int accumulate, void* stream) {
  if (!s) return YMS_ERR_INVALID;
  const yms_conv_dgrad_job j{*s, dz, dz_ld, dz_off, wpacked_t, dx, dx_ld, dx_off, accumulate};
  return args_ok(j) ? conv_solo(j, route_of(j), (hipStream_t)stream) : YMS_ERR_INVALID;
}

yms_status yms_conv_fwd_group(int njobs, const yms_conv_fwd_job* jobs, void* stream) {
  return conv_group<MODE_FWD>(njobs, jobs, stream, nullptr);
}
int yms_conv_fwd_group_launches(int njobs, const yms_conv_fwd_job* jobs) {
  int n = 0;
  return conv_group<MODE_FWD>(njobs, jobs, nullptr, &n) == YMS_OK ? n : -1;
}
yms_status yms_conv_dgrad_group(int njobs, const yms_conv_dgrad_job* jobs, void* stream) {
  return conv_group<MODE_DGRAD>(njobs, jobs, stream, nullptr);
}
int yms_conv_dgrad_group_launches(int njobs, const yms_conv_dgrad_job* jobs) {
  int n = 0;
  return conv_group<MODE_DGRAD>(njobs, jobs, nullptr, &n) == YMS_OK ? n : -1;
}

int yms_conv_dgrad_bnred_rows(const yms_conv_shape* s) {
  DirectGeo dg;
  if (!shape_ok(s) || s->cin % 8 != 0 || !conv_direct_geometry(s, 1, &dg, true)) return 0;
  return dg.grid;
}

yms_status yms_conv_dgrad_bnred(const yms_conv_shape* s, const void* dz, int dz_ld, int dz_off,
                                const void* wpacked_t, void* dx, int dx_ld, int dx_off, int accumulate,
                                const void* z, int z_ld, int z_off, const float* scale, const float* shift,
                                const float* mean_invstd, int act, float* ws, void* stream) {
  if (!shape_ok(s) || !dz || !wpacked_t || !dx || !z || !scale || !shift || !mean_invstd || !ws)
    return YMS_ERR_INVALID;
  if (!view_ok(dz_ld, dz_off, s->cout) || !view_ok(dx_ld, dx_off, s->cin) || !view_ok(z_ld, z_off, s->cin))
    return YMS_ERR_INVALID;
  if (act != YMS_ACT_NONE && act != YMS_ACT_SILU) return YMS_ERR_INVALID;
  DirectGeo dg;
  if (s->cin % 8 != 0 || !conv_direct_geometry(s, 1, &dg, true)) return YMS_ERR_UNSUPPORTED;
  const DirectBnRed b{z, z_ld, z_off, scale, shift, mean_invstd, act, ws};
  return conv_direct_launch(s, 1, dg, dz, dz_ld, dz_off, wpacked_t, dx, dx_ld, dx_off, nullptr, nullptr, 0, nullptr,
                            0, 0, nullptr, accumulate, (hipStream_t)stream, &b);
}

}  // extern "C"
