// bore_stream.hip -- the STREAMED flavour: float32 Dense stacks whose parameters do not fit one
// workgroup's LDS (mlp_layout.h) stay in global memory -- L2-resident in practice, 3.2 MB at
// 512-512-512 -- and pass through LDS in panels.  Serves bore_mlp_forward, bore_mlp_evaluate,
// bore_mlp_value_and_input_grad and bore_mlp_fit; an entry point comes here exactly when its own LDS
// check refuses the network for capacity (or BORE_STREAM=1 asks for it: tests run both flavours on
// the same inputs).  The acquisition side has entry points of its own, which stream ANY float32 network
// within the bounds: bore_stream_screen_topk / bore_stream_sample_screen_topk (the forward pass over the
// candidates, then the selection stage of bore_argmax.hip), bore_stream_lbfgsb_minimize (lbfgsb.h's state
// machines, one problem per wave, around the value + input-gradient pass of this file) and bore_stream_svgd_optimize
// (svgd_interact.h's particle interaction, one workgroup per model, around the same pass).
//
// Every matrix product of the path is one routine, stream_gemm: C[M x N] = sum_r A(i, r) B(r, j) with
// both operands in global memory, either of them read transposed.  A 64 x 128 output tile at a time:
// the workgroup stages a 64 x 32 panel of A and a 32 x 128 panel of B into LDS (double-buffered: the
// next panel's loads are in flight under the current panel's MFMAs, one barrier per panel), wave w owns
// rows [16 w, 16 w + 16) of the tile and keeps eight 16 x 16 accumulators (eight independent
// v_mfma_f32_16x16x4_f32 chains).  An output element is ONE fmaf chain over r in ascending order,
// whatever the tiling and whichever rows share the tile: a row alone gives the bits it gives in a batch,
// a model alone the bits it gives in a multi-model launch.  No float atomics anywhere.
//
// Activations and deltas of the current 64-row tile live in a stream-ordered device workspace
// (hipMallocAsync; at 8 x 512 x 64 rows they do not fit LDS), written once and read once per product.
// Data that one wave writes and another wave of the SAME workgroup reads (activations, deltas, theta
// after an Adam update) is handed over by __syncthreads(): a workgroup-scope release / acquire around
// the barrier.  No workgroup ever waits for another one.
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "host_common.h"
#include "lbfgsb.h"
#include "mlp_device.h"
#include "mlp_math.h"
#include "stream_restart.h"
#include "svgd_interact.h"

namespace bore {

constexpr int SKP = 32;          // reduction depth of a panel
constexpr int SNC = 128;         // output columns per pass: 8 accumulators per wave
constexpr int SROWS = BORE_BATCH_MAX;
constexpr int SLDA = SKP + 2;    // 2 * odd: the 16-row x 4-k operand fetch hits distinct banks
constexpr int SLDB = SNC + 16;   // the four k-rows of an operand fetch land 16 banks apart
constexpr long long STREAM_WS_BYTES = 64ll << 20;  // the rows kernels' workspace per call (one tile per model at least)

struct StreamLds {
  float a[2][SROWS * SLDA];
  float b[2][SKP * SLDB];
  int layout[(sizeof(MlpLayout) + 3) / 4];
  int pre[BORE_MAX_LAYERS + 2];  // pre[l] = w[0] + .. + w[l-1]: where A_l / D_l start in the workspace
  float zt[SROWS];               // labels of the tile rows (fit, evaluate)
  float red[BORE_THREADS / 64];
};

// Floats of workspace one workgroup needs: A_0..A_n and D_0..D_n of a 64-row tile.
static inline size_t stream_tile_floats(const MlpLayout &L) {
  size_t s = 0;
  for (int l = 0; l <= L.n_layers; ++l) s += (size_t)L.w[l];
  return 2 * SROWS * s;
}

__device__ __forceinline__ const MlpLayout &stream_begin(StreamLds &S, const MlpLayout &Lk) {
  const int *src = reinterpret_cast<const int *>(&Lk);
  for (int i = threadIdx.x; i < (int)(sizeof(MlpLayout) / 4); i += blockDim.x) S.layout[i] = src[i];
  if (threadIdx.x == 0) {
    int s = 0;
    for (int l = 0; l <= Lk.n_layers; ++l) {
      S.pre[l] = s;
      s += Lk.w[l];
    }
    S.pre[Lk.n_layers + 1] = s;
  }
  __syncthreads();
  return *reinterpret_cast<const MlpLayout *>(S.layout);
}

// C[i][j] = init(i, j) + sum_{r < R} A(i, r) B(r, j) for i < M, j < N, handed to epi(i, j, value).
//   A(i, r) = Ag[i * lda + r]  (A_T: Ag[r * lda + i]);   B(r, j) = Bg[r * ldb + j]  (B_T: Bg[j * ldb + r])
// Called by the whole workgroup with the same arguments; ends with a barrier, after which what the
// epilogues wrote is visible to every wave of the workgroup.
template <bool A_T, bool B_T, typename Init, typename Epi>
__device__ __forceinline__ void stream_gemm(StreamLds &S, const int M, const int N, const int R, const float *Ag,
                                            const int lda, const float *Bg, const int ldb, Init init, Epi epi) {
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, m16 = lane & 15, q4 = lane >> 4;
  constexpr int NA = SROWS * SKP / BORE_THREADS, NB = SKP * SNC / BORE_THREADS;
  const int n_panels = (R + SKP - 1) / SKP;
  for (int i0 = 0; i0 < M; i0 += SROWS)
    for (int j0 = 0; j0 < N; j0 += SNC) {
      float ra[NA], rb[NB];
      auto fetch = [&](const int r0) {  // this work-item's share of the panels at r0: global -> registers
#pragma unroll
        for (int u = 0; u < NA; ++u) {
          const int e = tid + BORE_THREADS * u;
          const int i = i0 + (A_T ? (e & (SROWS - 1)) : e / SKP), r = r0 + (A_T ? e / SROWS : (e & (SKP - 1)));
          ra[u] = (i < M && r < R) ? Ag[A_T ? r * lda + i : i * lda + r] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < NB; ++u) {
          const int e = tid + BORE_THREADS * u;
          const int j = j0 + (B_T ? e / SKP : (e & (SNC - 1))), r = r0 + (B_T ? (e & (SKP - 1)) : e / SNC);
          rb[u] = (j < N && r < R) ? Bg[B_T ? j * ldb + r : r * ldb + j] : 0.f;
        }
      };
      auto park = [&](const int buf) {  // registers -> LDS
#pragma unroll
        for (int u = 0; u < NA; ++u) {
          const int e = tid + BORE_THREADS * u;
          const int i = A_T ? (e & (SROWS - 1)) : e / SKP, r = A_T ? e / SROWS : (e & (SKP - 1));
          S.a[buf][i * SLDA + r] = ra[u];
        }
#pragma unroll
        for (int u = 0; u < NB; ++u) {
          const int e = tid + BORE_THREADS * u;
          const int j = B_T ? e / SKP : (e & (SNC - 1)), r = B_T ? (e & (SKP - 1)) : e / SNC;
          S.b[buf][r * SLDB + j] = rb[u];
        }
      };
      const int rows_here = min(SROWS, M - i0), ncb = (min(SNC, N - j0) + 15) >> 4;
      const bool mine = 16 * wv < rows_here;  // (a wave without rows still stages panels and meets the barriers)
      f32x4 acc[SNC / 16];
#pragma unroll
      for (int cb = 0; cb < SNC / 16; ++cb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = i0 + 16 * wv + 4 * q4 + r, j = j0 + 16 * cb + m16;
          acc[cb][r] = (mine && cb < ncb && i < M && j < N) ? init(i, j) : 0.f;
        }
      fetch(0);
      park(0);
      __syncthreads();
      for (int p = 0; p < n_panels; ++p) {
        const int buf = p & 1;
        if (p + 1 < n_panels) fetch((p + 1) * SKP);
        if (mine) {
          const int kcs = (min(SKP, R - p * SKP) + 3) >> 2;
          const float *ap = S.a[buf] + (16 * wv + m16) * SLDA + q4;
          const float *bp = S.b[buf] + q4 * SLDB + m16;
          for (int kc = 0; kc < kcs; ++kc) {
            const float av = ap[4 * kc];
#pragma unroll
            for (int cb = 0; cb < SNC / 16; ++cb)
              if (cb < ncb) acc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bp[4 * kc * SLDB + 16 * cb], acc[cb], 0, 0, 0);
          }
        }
        if (p + 1 < n_panels) park(buf ^ 1);
        __syncthreads();
      }
      if (mine) {
#pragma unroll
        for (int cb = 0; cb < SNC / 16; ++cb)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int i = i0 + 16 * wv + 4 * q4 + r, j = j0 + 16 * cb + m16;
            if (cb < ncb && i < M && j < N) epi(i, j, acc[cb][r]);
          }
      }
    }
  __syncthreads();
}

// A_l = act_l(A_{l-1} W_l + b_l), l = 1..n, for the nr rows of the tile whose inputs sit in A_0.
template <bool FIT>
__device__ __forceinline__ void stream_forward(StreamLds &S, const MlpLayout &L, const float *th, float *ws, const int nr,
                                               const bool keep_logits) {
  const int n = L.n_layers;
  for (int l = 1; l <= n; ++l) {
    const int K = L.w[l - 1], Nw = L.w[l];
    const float *Ain = ws + SROWS * S.pre[l - 1];
    float *Aout = ws + SROWS * S.pre[l];
    const float *bias = th + L.goff_b[l];
    const int act = (keep_logits && l == n) ? (int)BORE_ACT_LINEAR : L.act[l];
    stream_gemm<false, false>(
        S, nr, Nw, K, Ain, K, th + L.goff_w[l], Nw, [](int, int) { return 0.f; },
        [&](const int i, const int j, const float v) { Aout[i * Nw + j] = act_fwd<FIT>(act, v + bias[j]); });
  }
}

// D_{l-1} = (D_l W_l^T) .* act'_{l-1}(A_{l-1}) for the nr rows of the tile (l == 1: no activation below).
__device__ __forceinline__ void stream_backward_layer(StreamLds &S, const MlpLayout &L, const float *th, float *ws,
                                                      const int nr, const int l) {
  const int K = L.w[l - 1], Nw = L.w[l];
  const float *Din = ws + SROWS * (S.pre[L.n_layers + 1] + S.pre[l]);
  float *Dout = ws + SROWS * (S.pre[L.n_layers + 1] + S.pre[l - 1]);
  const float *Aprev = ws + SROWS * S.pre[l - 1];
  const int act = L.act[l - 1];
  stream_gemm<false, true>(
      S, nr, K, Nw, Din, Nw, th + L.goff_w[l], Nw, [](int, int) { return 0.f; },
      [&](const int i, const int j, const float v) {
        Dout[i * K + j] = l > 1 ? v * act_grad(act, Aprev[i * K + j]) : v;
      });
}

// Fixed-order sum over a workgroup of BORE_THREADS: a fixed tree over the lanes of a wave, then the four waves in
// order.  Called by the whole workgroup; every work-item gets the value.  Ends with a barrier.
__device__ __forceinline__ float stream_wg_sum(StreamLds &S, float v) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) S.red[threadIdx.x >> 6] = v;
  __syncthreads();
  const float total = ((S.red[0] + S.red[1]) + S.red[2]) + S.red[3];
  __syncthreads();
  return total;
}

// sum over l of l2_w[l] |W_l|^2 + l2_b[l] |b_l|^2: per-lane strided sums, then stream_wg_sum.  Called by the whole
// workgroup after a barrier; every work-item gets the value.
__device__ __forceinline__ float stream_penalty(StreamLds &S, const MlpLayout &L, const float *th) {
  const int tid = threadIdx.x, nthr = blockDim.x;
  float reg = 0.f;
  for (int l = 1; l <= L.n_layers; ++l) {
    const float lw = L.l2_w[l], lb = L.l2_b[l];
    if (lw != 0.f)
      for (int p = tid; p < L.w[l - 1] * L.w[l]; p += nthr) {
        const float w = th[L.goff_w[l] + p];
        reg = fmaf(lw * w, w, reg);
      }
    if (lb != 0.f)
      for (int p = tid; p < L.w[l]; p += nthr) {
        const float w = th[L.goff_b[l] + p];
        reg = fmaf(lb * w, w, reg);
      }
  }
  return stream_wg_sum(S, reg);
}

// ---------------------------------------------------------------------------
// rows: forward, and value + input gradient.  Grid (model, row tiles).
// ---------------------------------------------------------------------------
struct StreamRowArgs {
  MlpLayout L;
  const float *theta;
  const float *Xf;
  const double *Xd;
  float *out;
  double *grad;
  long long n_rows;
  int x_shared, transform;
  float sign;
  float *ws;
  long long ws_stride;  // floats per workgroup
};

// Value and input gradient of T(sign f(x)) for the nr rows of the tile whose inputs sit in A_0: the forward pass,
// the objective's value -- row r's into vals[r] -- and output delta, the backward pass down to D_0.  Called by the
// whole workgroup after a barrier behind the writes of A_0; ends with a barrier (stream_gemm's), after which D_0 and
// vals are visible to every wave.  ONE definition of the sequence for the rows kernel and the restart kernel below:
// their values and gradients are the same bits.
__device__ __forceinline__ void stream_value_and_grad(StreamLds &S, const MlpLayout &L, const float *th, float *ws,
                                                      const int nr, const int transform, const float sign,
                                                      const float *An, float *vals) {
  const int tid = threadIdx.x, n = L.n_layers;
  stream_forward<false>(S, L, th, ws, nr, false);
  float *Dn = ws + SROWS * (S.pre[n + 1] + S.pre[n]);
  if (tid < nr) {
    const float f = An[tid];
    const float u = sign * f;
    float T, dT;
    objective_transform(transform, u, T, dT);
    vals[tid] = T;
    Dn[tid] = sign * dT * act_grad(L.act[n], f);
  }
  __syncthreads();
  for (int l = n; l >= 1; --l) stream_backward_layer(S, L, th, ws, nr, l);
}

template <bool WITH_GRAD>
__global__ __launch_bounds__(BORE_THREADS) void stream_rows_kernel(const StreamRowArgs a) {
  __shared__ StreamLds S;
  const MlpLayout &L = stream_begin(S, a.L);
  const int tid = threadIdx.x, nthr = blockDim.x;
  const long long model = blockIdx.x;
  const int n = L.n_layers, D = L.w[0];
  const float *th = a.theta + model * L.P;
  float *ws = a.ws + (model * gridDim.y + blockIdx.y) * a.ws_stride;
  const long long xoff = a.x_shared ? 0 : model * a.n_rows * D;
  float *out = a.out + model * a.n_rows;
  const long long n_tiles = (a.n_rows + SROWS - 1) / SROWS;
  float *A0 = ws, *An = ws + SROWS * S.pre[n];
  for (long long t = blockIdx.y; t < n_tiles; t += gridDim.y) {
    const long long row0 = t * SROWS;
    const int nr = (int)min((long long)SROWS, a.n_rows - row0);
    for (int i = tid; i < nr * D; i += nthr)
      A0[i] = WITH_GRAD ? (float)a.Xd[xoff + row0 * D + i]  // Keras autocast fp64 -> fp32
                        : a.Xf[xoff + row0 * D + i];
    __syncthreads();
    if constexpr (!WITH_GRAD) {
      stream_forward<false>(S, L, th, ws, nr, false);
      if (tid < nr) out[row0 + tid] = An[tid];
    } else {
      stream_value_and_grad(S, L, th, ws, nr, a.transform, a.sign, An, out + row0);
      const float *D0 = ws + SROWS * S.pre[n + 1];
      double *grad = a.grad + (model * a.n_rows + row0) * D;
      for (int i = tid; i < nr * D; i += nthr) grad[i] = (double)D0[i];
    }
    __syncthreads();  // (the next tile overwrites the workspace)
  }
}

// ---------------------------------------------------------------------------
// screening: the forward pass over fp64 candidates (in memory, or row i of bore_uniform_candidates' counter stream
// recomputed where it is read) into a prediction buffer, then one selection workgroup per model -- the selection
// stage of bore_argmax.hip (screen_select) with an LDS carve of its own: keys and, sampled, the box; no theta.
// ---------------------------------------------------------------------------
struct StreamSampleArgs {
  unsigned long long seed;
  long long model0, draw;
  int sampled;
  BoxArgs box;
};

// Candidate element (row, d) of `model` in fp64: read, or recomputed exactly as candidates_kernel writes it.
struct StreamCandidates {
  const double *X;
  const double *blo, *bhi;  // LDS copy of the box (indexed per lane)
  unsigned long long cbase;
  int D, sampled;
  __device__ __forceinline__ double operator()(const long long row, const int d) const {
    if (sampled) {
      const long long i = row * D + d;
      const unsigned long long r = mix64(cbase + 0x8CB92BA72F3D8DD7ULL * (unsigned long long)(i + 1));
      const double u = (double)(r >> 11) * (1.0 / 9007199254740992.0);
      return blo[d] + (bhi[d] - blo[d]) * u;
    }
    return X[row * D + d];
  }
};

__device__ __forceinline__ StreamCandidates stream_candidates(const StreamSampleArgs &sp, const double *X,
                                                              const long long n_samples, const int x_shared, const int D,
                                                              double *box_lds) {
  const long long model = blockIdx.x;
  StreamCandidates c;
  c.D = D;
  c.sampled = sp.sampled;
  c.X = sp.sampled ? nullptr : X + (x_shared ? 0 : model * n_samples * D);
  c.blo = box_lds;
  c.bhi = box_lds + D;
  c.cbase = sp.sampled ? candidate_base(sp.seed, sp.model0 + model, sp.draw) : 0ULL;
  if (sp.sampled && (int)threadIdx.x < D) {
    box_lds[threadIdx.x] = sp.box.lo[threadIdx.x];
    box_lds[D + threadIdx.x] = sp.box.hi[threadIdx.x];
  }
  __syncthreads();
  return c;
}

// The rows kernel's forward form (its geometry and workspace: StreamRowArgs, n_rows = the candidates, Xd = their
// rows) with A_0 filled from the fp64 candidates.
__global__ __launch_bounds__(BORE_THREADS) void stream_screen_pred_kernel(const StreamRowArgs a, const StreamSampleArgs sp) {
  __shared__ StreamLds S;
  __shared__ double box_lds[2 * BORE_DIM_MAX];
  const MlpLayout &L = stream_begin(S, a.L);
  const int tid = threadIdx.x, nthr = blockDim.x;
  const long long model = blockIdx.x;
  const int n = L.n_layers, D = L.w[0];
  const StreamCandidates cand = stream_candidates(sp, a.Xd, a.n_rows, a.x_shared, D, box_lds);
  const float *th = a.theta + model * L.P;
  float *ws = a.ws + (model * gridDim.y + blockIdx.y) * a.ws_stride;
  float *out = a.out + model * a.n_rows;
  const int n_tiles = (int)((a.n_rows + SROWS - 1) / SROWS);  // (n_rows <= BORE_STREAM_MAX_SAMPLES)
  float *A0 = ws, *An = ws + SROWS * S.pre[n];
  for (int t = blockIdx.y; t < n_tiles; t += gridDim.y) {
    const int row0 = t * SROWS;
    const int nr = min(SROWS, (int)a.n_rows - row0);
    for (int i = tid; i < nr * D; i += nthr) {
      const int r = i / D;
      A0[i] = (float)cand(row0 + r, i - r * D);  // Keras autocast fp64 -> fp32
    }
    __syncthreads();
    stream_forward<false>(S, L, th, ws, nr, false);
    if (tid < nr) out[row0 + tid] = An[tid];
    __syncthreads();  // (the next tile overwrites the workspace)
  }
}

struct StreamSelectArgs {
  const double *X;
  const float *pred;
  double *x0;
  int *idx;
  long long n_samples;
  int x_shared, R, n_pad, D;
};

__global__ __launch_bounds__(BORE_THREADS) void stream_select_kernel(const StreamSelectArgs a, const StreamSampleArgs sp) {
  extern __shared__ float smem[];
  __shared__ double box_lds[2 * BORE_DIM_MAX];
  const long long model = blockIdx.x;
  // (the keys are 8-byte values: the dynamic region may start on a 4-byte boundary behind the static one)
  unsigned long long *keys =
      reinterpret_cast<unsigned long long *>(reinterpret_cast<char *>(smem) + ((8 - ((size_t)smem & 7)) & 7));
  const StreamCandidates cand = stream_candidates(sp, a.X, a.n_samples, a.x_shared, a.D, box_lds);
  const int tid = threadIdx.x, nthr = blockDim.x;
  screen_keys_from_pred(tid, nthr, keys, a.pred + model * a.n_samples, (int)a.n_samples);
  screen_select(tid, nthr, keys, (int)a.n_samples, a.n_pad, a.R, a.D, a.idx + model * a.R,
                a.x0 + model * (long long)a.R * a.D, cand);
}

// ---------------------------------------------------------------------------
// restarts: bound-constrained L-BFGS-B (lbfgsb.h) around a streamed value + input gradient pass -- ONE driver,
// stream_restart_drive, for the Dense kernel below and the recurrent one (bore_lstm_stream.hip).  Grid (model,
// workgroups of the model).  One problem per wave at a time, all 64 lanes on it (lbfgsb::Coop); wave w of workgroup b
// runs the model's problems (b + k gridDim.y) * waves + w, k = 0, 1, .. one after another.  A ROUND: every wave with a
// live problem advances its state machine to the next request for f and g (finishing problems and taking the next on
// the way) and puts the point into ITS row of the flavour's point buffer (`put`); then the whole workgroup runs ONE
// value + gradient pass over the `waves` rows (`pass`), and every wave takes f and g of its row (`read`).  The passes
// are full of barriers, so whether a round's pass runs is ONE workgroup-uniform value -- the waves' requests, OR-ed
// through LDS behind a barrier -- and every wave, with or without a problem, runs every pass until that value is 0 or
// the round cap (from maxfun, as lbfgsb_body's) is reached.  Rows of waves without a request keep their last point
// (zeros at first, from `prepare`, which runs ahead of the first barrier): finite, and no row's bits depend on its
// neighbours.  The optimiser's vectors stay in LDS (LB_LANES_SYNC waits for LDS alone); the points, values and
// gradients cross global memory between waves of ONE workgroup, handed over by __syncthreads().  No workgroup waits
// for another; no float atomics.
// ---------------------------------------------------------------------------
struct RestartArgs {  // what the restart kernels of both flavours take beside their network
  const double *x0;
  double *x, *fun, *jac;
  int *info;
  BoxArgs box;
  int nbd[BORE_DIM_MAX];
  lbfgsb::Options opt;
  int R, transform, waves;  // waves: how many of the four hold a problem (the workspaces that fit LDS)
  long long max_rounds;
  float sign;
  float *ws;
  long long ws_stride;  // floats per workgroup
  RestartLds lds;       // the dynamic LDS (stream_restart.h)
};

// put(wv, lane, x): the wave's fp64 point x[D] into its row;  pass(): the workgroup's value + gradient pass;
// read(wv, lane, f, g): f and g[D] of the wave's row.
template <class Prepare, class Put, class Pass, class Read>
__device__ __forceinline__ void stream_restart_drive(const RestartArgs &a, const int D, Prepare prepare, Put put,
                                                     Pass pass, Read read) {
  extern __shared__ float smem[];
  const int tid = threadIdx.x;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const long long model = blockIdx.x;
  const int NW = a.waves;
  // (fp64 LDS reads merge into ds_read_b128: every base on a 16-byte boundary, lbfgsb.h)
  float *dyn = reinterpret_cast<float *>(reinterpret_cast<char *>(smem) + ((16 - ((size_t)smem & 15)) & 15));
  double *blo = reinterpret_cast<double *>(dyn + a.lds.o_box), *bhi = blo + ((D + 1) & ~1);
  int *bnbd = reinterpret_cast<int *>(bhi + ((D + 1) & ~1));
  int *vote = reinterpret_cast<int *>(dyn + a.lds.o_vote);
  float *slot = dyn + a.lds.o_prob + (size_t)(wv < NW ? wv : 0) * a.lds.prob_floats;
  lbfgsb::State *parked = reinterpret_cast<lbfgsb::State *>(slot);
  const lbfgsb::Work wk = lbfgsb::make_work(reinterpret_cast<double *>(slot + a.lds.o_dw),
                                            reinterpret_cast<int *>(slot + a.lds.o_iw), D, a.opt.m);
  const lbfgsb::Coop cp{lane, 64};
  if (tid < D) {
    blo[tid] = a.box.lo[tid];
    bhi[tid] = a.box.hi[tid];
    bnbd[tid] = a.nbd[tid];
  }
  prepare();
  __syncthreads();

  lbfgsb::State st;
  int k = 0;           // problems this wave has taken
  long long q = 0;     // the live one: x0 / x / fun / jac / info of restart q of the model
  bool live = false;
  // the wave's next problem, if the model has one left for it: a zeroed workspace (what the optimiser counts on), init
  auto take = [&]() {
    q = ((long long)blockIdx.y + (long long)k * gridDim.y) * NW + wv;
    ++k;
    live = wv < NW && q < a.R;
    if (!live) return;
    float4 *b4 = reinterpret_cast<float4 *>(slot);
    for (int i = lane; i < a.lds.prob_floats / 4; i += 64) b4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    wave_lds_sync();
    lbfgsb::lbfgsb_init(st, wk, D, a.opt.m, a.x0 + (model * a.R + q) * D, blo, bhi, bnbd, cp);
    wave_lds_sync();
  };
  auto report = [&]() {  // bore_lbfgsb_minimize's layout and semantics
    const long long p = model * a.R + q;
    for (int d = lane; d < D; d += 64) {
      a.x[p * D + d] = wk.x[d];
      a.jac[p * D + d] = wk.g[d];
    }
    if (lane == 0) {
      a.fun[p] = st.f;
      int *inf = a.info + p * 5;
      inf[0] = st.nit; inf[1] = st.nfev; inf[2] = st.status; inf[3] = st.task; inf[4] = st.msg;
    }
  };
  take();
  for (long long round = 0; round < a.max_rounds; ++round) {
    int need = 0;
    while (live) {  // (wave-uniform: the 64 lanes hold the same State)
      const int rc = __builtin_amdgcn_readfirstlane(lbfgsb::lbfgsb_advance<true>(st, wk, blo, bhi, bnbd, a.opt, cp));
      if (rc == lbfgsb::LB_NEED_FG) {
        put(wv, lane, wk.x);
        need = 1;
        break;
      }
      report();
      take();
    }
    // (the State rests in LDS over the pass: the products want the registers)
    if (need) *parked = st;
    if (lane == 0) vote[wv] = need;
    __syncthreads();  // the votes; the points
    if (!__builtin_amdgcn_readfirstlane(vote[0] | vote[1] | vote[2] | vote[3])) break;  // (ONE value for the workgroup)
    pass();
    if (need) {
      st = *parked;
      read(wv, lane, st.f, wk.g);
      wave_lds_sync();
    }
  }
  // The round cap (cannot happen with a sane cap): what is left is REPORTED, unoptimised, with status 2 -- never dropped.
  while (live) {
    if (st.stage != lbfgsb::S_FINISHED) {
      st.status = 2;
      st.task = lbfgsb::T_STOP;
      st.msg = lbfgsb::M_MAXFUN;
    }
    report();
    take();
  }
}

// The Dense flavour plugs in: the points as float rows of A_0 (Keras autocast), stream_value_and_grad over the four
// rows (the rows kernel's sequence, the same bits), f from A_n and g from D_0.
struct StreamLbfgsbArgs {
  MlpLayout L;
  const float *theta;
  RestartArgs r;
};

__global__ __launch_bounds__(BORE_THREADS) void stream_lbfgsb_kernel(const StreamLbfgsbArgs a) {
  __shared__ StreamLds S;
  const MlpLayout &L = stream_begin(S, a.L);
  const long long model = blockIdx.x;
  const int n = L.n_layers, D = L.w[0];
  const float *th = a.theta + model * L.P;
  float *ws = a.r.ws + (model * gridDim.y + blockIdx.y) * a.r.ws_stride;
  float *A0 = ws, *An = ws + SROWS * S.pre[n];
  const float *D0 = ws + SROWS * S.pre[n + 1];
  stream_restart_drive(
      a.r, D,
      [&] {  // (rows of waves that never ask)
        for (int i = threadIdx.x; i < BORE_THREADS / 64 * D; i += BORE_THREADS) A0[i] = 0.f;
      },
      [&](const int wv, const int lane, const double *x) {
        for (int d = lane; d < D; d += 64) A0[wv * D + d] = (float)x[d];  // Keras autocast fp64 -> fp32
      },
      [&] { stream_value_and_grad(S, L, th, ws, BORE_THREADS / 64, a.r.transform, a.r.sign, An, An); },  // (A_n: f, then T(sign f))
      [&](const int wv, const int lane, double &f, double *g) {
        f = (double)An[wv];
        for (int d = lane; d < D; d += 64) g[d] = (double)D0[wv * D + d];
      });
}

// ---------------------------------------------------------------------------
// SVGD batch acquisition (bore_svgd.hip's statement of it): ONE workgroup per model, every iteration of every
// particle in one launch.  The particle state -- x, fg, grad, hist fp64 [n][D], f and zeta fp64 [n], the radix
// select's scratch -- stays in the dynamic LDS beside the panels for the whole launch: svgd_big_kernel's carve
// without theta and without the activation tile, and no n x n matrix for any n (svgd_interact.h forms its entries
// on the fly: ONE definition of the interaction for both kernels).  Value and input gradient of the particles,
// 64 at a time, are the rows kernel's sequence (stream_value_and_grad: the same bits), sign +1: SVGD climbs
// transform(f).  The points, values and gradients cross global memory between waves of ONE workgroup, handed over
// by __syncthreads().  No workgroup waits for another; no float atomics.
// ---------------------------------------------------------------------------
struct StreamSvgdArgs {
  MlpLayout L;
  const float *theta;
  const double *x_init;
  double *x_out;
  double lo[BORE_DIM_MAX], hi[BORE_DIM_MAX];
  int clip, n, n_iter, transform, distortion;
  double step, alpha, eps, tau, length_scale, dparam;
  float *ws;
  long long ws_stride;  // floats per workgroup
  // dynamic LDS (float offsets from its 16-byte aligned start; every region a multiple of 16 bytes)
  int o_x, o_fg, o_grad, o_hist, o_f, o_sel;
};

__global__ __launch_bounds__(BORE_THREADS) void stream_svgd_kernel(const StreamSvgdArgs a) {
  __shared__ StreamLds S;
  extern __shared__ float smem[];
  const MlpLayout &L = stream_begin(S, a.L);
  const int tid = threadIdx.x;
  const long long model = blockIdx.x;
  const int nl = L.n_layers, D = L.w[0], n = a.n, nD = n * D;
  const float *th = a.theta + model * L.P;
  float *ws = a.ws + model * a.ws_stride;
  float *A0 = ws, *An = ws + SROWS * S.pre[nl];
  const float *D0 = ws + SROWS * S.pre[nl + 1];
  float *dyn = reinterpret_cast<float *>(reinterpret_cast<char *>(smem) + ((16 - ((size_t)smem & 15)) & 15));
  double *x = reinterpret_cast<double *>(dyn + a.o_x);
  double *fg = reinterpret_cast<double *>(dyn + a.o_fg);
  double *grad = reinterpret_cast<double *>(dyn + a.o_grad);
  double *hist = reinterpret_cast<double *>(dyn + a.o_hist);
  double *f = reinterpret_cast<double *>(dyn + a.o_f), *zeta = f + n;
  unsigned *sel = reinterpret_cast<unsigned *>(dyn + a.o_sel);  // [256] bins + [8] scratch
  for (int e = tid; e < nD; e += BORE_THREADS) x[e] = a.x_init[model * nD + e];
  __syncthreads();
  for (int it = 0; it < a.n_iter; ++it) {
    const double gamma = svgd_gamma(x, n, D, a.length_scale, sel);
    // value and input gradient of every particle, 64 rows of the workspace tile at a time
    for (int c0 = 0; c0 < n; c0 += SROWS) {
      const int nr = min(SROWS, n - c0);
      for (int i = tid; i < nr * D; i += BORE_THREADS) A0[i] = (float)x[c0 * D + i];  // Keras autocast fp64 -> fp32
      __syncthreads();
      stream_value_and_grad(S, L, th, ws, nr, a.transform, 1.f, An, An);  // (A_n: f, then T(f))
      for (int i = tid; i < nr * D; i += BORE_THREADS) fg[c0 * D + i] = (double)D0[i];
      for (int i = tid; i < nr; i += BORE_THREADS) f[c0 + i] = (double)An[i];
      __syncthreads();  // (the next chunk overwrites the workspace)
    }
    svgd_zeta(f, zeta, n, a.distortion, a.dparam);
    svgd_drive_repulsion(x, fg, zeta, grad, n, D, gamma, a.tau);
    svgd_step_clip(x, grad, hist, nD, D, it == 0, a.step, a.alpha, a.eps, a.clip, a.lo, a.hi);
  }
  for (int e = tid; e < nD; e += BORE_THREADS) a.x_out[model * nD + e] = x[e];
}

// ---------------------------------------------------------------------------
// evaluate: one workgroup per model over all N rows
// ---------------------------------------------------------------------------
struct StreamEvalArgs {
  MlpLayout L;
  const float *theta, *X, *z;
  float *loss, *acc;
  long long N;
  float *ws;
  long long ws_stride;
  const float *sw;  // sample weights [n_models][N] (the WEIGHTED instantiation alone reads them)
};

// WEIGHTED: a.sw [n_models][N] weighs each row's loss term; the divisor stays N, the accuracy stays unweighted.
template <bool WEIGHTED>
__global__ __launch_bounds__(BORE_THREADS) void stream_evaluate_kernel(const StreamEvalArgs a) {
  __shared__ StreamLds S;
  const MlpLayout &L = stream_begin(S, a.L);
  const int tid = threadIdx.x, nthr = blockDim.x;
  const long long model = blockIdx.x;
  const int n = L.n_layers, D = L.w[0];
  const float *th = a.theta + model * L.P;
  float *ws = a.ws + model * a.ws_stride;
  const float *X = a.X + model * a.N * D;
  const float *z = a.z + model * a.N;
  float *A0 = ws, *An = ws + SROWS * S.pre[n];
  float lsum = 0.f, csum = 0.f;  // of this work-item's row slot, tile after tile
  for (long long row0 = 0; row0 < a.N; row0 += SROWS) {
    const int nr = (int)min((long long)SROWS, a.N - row0);
    for (int i = tid; i < nr * D; i += nthr) A0[i] = X[row0 * D + i];
    __syncthreads();
    stream_forward<false>(S, L, th, ws, nr, true);
    if (tid < nr) {
      const float x = An[tid];
      const float zz = z[row0 + tid];
      if constexpr (WEIGHTED) lsum += bce_loss_weighted(x, zz, a.sw[model * a.N + row0 + tid]);
      else lsum += bce_loss(x, zz);
      const float o = L.act[n] == BORE_ACT_SIGMOID ? sigmoid_stable(x) : x;
      csum += accuracy_hit(o, zz);
    }
    __syncthreads();
  }
  const float reg = L.any_l2 ? stream_penalty(S, L, th) : 0.f;
  lsum = wave_sum(lsum);  // (rows live in the first wave's slots only)
  csum = wave_sum(csum);
  if (tid == 0) {
    a.loss[model] = lsum / (float)a.N + reg;
    a.acc[model] = csum / (float)a.N;
  }
}

// ---------------------------------------------------------------------------
// fit: ONE workgroup per model, every Adam step of the call in one launch
// ---------------------------------------------------------------------------
struct StreamFitArgs {
  MlpLayout L;
  float *theta, *am, *av;
  long long *at;
  const float *X, *z;
  const int *perm;  // [models][epochs][N]: the caller's, or drawn by shuffle_kernel in front of this launch
  float *epoch_loss;
  int N, epochs, B;
  float lr, beta1, beta2, eps;
  float *ws;
  long long ws_stride;  // floats per model: the tile's A / D, then (B > 64) the gradient sums [P]
  long long o_g;
  const float *sw;  // sample weights [n_models][N] (the WEIGHTED instantiation alone reads them)
};

// WEIGHTED: a.sw [n_models][N], a sample weight per row: the row's loss term and d loss / d logit are scaled by it, the
// divisor of the batch mean stays the row count (the weighted fit of bore_hip.hip's generic flavour, streamed).
template <bool WEIGHTED>
__global__ __launch_bounds__(BORE_THREADS) void stream_fit_kernel(const StreamFitArgs a) {
  __shared__ StreamLds S;
  const MlpLayout &L = stream_begin(S, a.L);
  const int tid = threadIdx.x, nthr = blockDim.x;
  const long long model = blockIdx.x;
  const int n = L.n_layers, D = L.w[0], N = a.N, P = L.P;
  float *th = a.theta + model * P, *mg = a.am + model * P, *vg = a.av + model * P;
  const float *Xg = a.X + model * (long long)N * D;
  const float *zg = a.z + model * (long long)N;
  [[maybe_unused]] const float *swg = WEIGHTED ? a.sw + model * (long long)N : nullptr;
  float *ws = a.ws + model * a.ws_stride;
  float *gsum = ws + a.o_g;  // weight-gradient sums carried between the sub-tiles of a batch of more than 64 rows
  float *A0 = ws, *An = ws + SROWS * S.pre[n];
  float *Dn = ws + SROWS * (S.pre[n + 1] + S.pre[n]);

  const long long t0 = a.at[model];
  AdamClock clock(a.beta1, a.beta2, t0);
  const float omb1 = 1.f - a.beta1, omb2 = 1.f - a.beta2;
  const int steps = (N + a.B - 1) / a.B;
  float reg = L.any_l2 ? stream_penalty(S, L, th) : 0.f;  // penalty of the weights the next step's loss sees

  for (int e = 0; e < a.epochs; ++e) {
    const int *perm = a.perm + (model * a.epochs + e) * (long long)N;
    float eloss = 0.f;  // of this work-item's row slot
    float ereg = 0.f;   // penalty x rows, step after step (the same in every work-item)
    for (int s = 0; s < steps; ++s) {
      const int row0 = s * a.B;
      const int nb = min(a.B, N - row0);
      const float inv_nb = fit_rcp((float)nb);
      const float alpha = clock.advance(a.lr, a.beta1, a.beta2);
      if (L.any_l2) ereg += reg * (float)nb;
      const int nsub = (nb + SROWS - 1) / SROWS;
      for (int sub = 0; sub < nsub; ++sub) {
        const int r0 = row0 + sub * SROWS;
        const int nr = min(SROWS, nb - sub * SROWS);
        const bool first_sub = sub == 0, last_sub = sub + 1 == nsub;
        // ---- gather, forward, loss ----
        for (int i = tid; i < nr * D; i += nthr) {
          const int r = i / D, d = i - r * D;
          A0[i] = Xg[(long long)perm[r0 + r] * D + d];
        }
        if (tid < nr) S.zt[tid] = zg[perm[r0 + tid]];
        [[maybe_unused]] float wrow = 0.f;  // (WEIGHTED) this work-item's row's weight: requested here, used at the loss
        if constexpr (WEIGHTED)
          if (tid < nr) wrow = swg[perm[r0 + tid]];
        __syncthreads();
        stream_forward<true>(S, L, th, ws, nr, true);
        if (tid < nr) {  // loss and d loss / d logit
          const float x = An[tid];
          const float zz = S.zt[tid];
          if constexpr (WEIGHTED) Dn[tid] = (fit_bce_weighted(x, zz, wrow, true, eloss) * inv_nb) * wrow;
          else Dn[tid] = fit_bce(x, zz, true, eloss) * inv_nb;
        }
        __syncthreads();
        // ---- per layer, descending: D_{l-1} from the OLD W_l, then dW_l = A_{l-1}^T D_l and its Adam update ----
        for (int l = n; l >= 1; --l) {
          if (l > 1) stream_backward_layer(S, L, th, ws, nr, l);
          const int K = L.w[l - 1], Nw = L.w[l];
          const float *Aprev = ws + SROWS * S.pre[l - 1];
          const float *Dl = ws + SROWS * (S.pre[n + 1] + S.pre[l]);
          const int gw = L.goff_w[l], gb = L.goff_b[l];
          const float l2w = L.l2_w[l], l2b = L.l2_b[l];
          stream_gemm<true, false>(
              S, K, Nw, nr, Aprev, K, Dl, Nw,
              [&](const int i, const int j) { return first_sub ? 0.f : gsum[gw + i * Nw + j]; },
              [&](const int i, const int j, const float v) {
                const int p = gw + i * Nw + j;
                if (!last_sub) {
                  gsum[p] = v;
                  return;
                }
                const float w = th[p];
                float g = v, mm = mg[p], vv = vg[p];
                if (l2w != 0.f) g = fmaf(2.f * l2w, w, g);
                th[p] = adam_update(w, g, mm, vv, alpha, omb1, omb2, a.eps);
                mg[p] = mm;
                vg[p] = vv;
              });
          for (int j = tid; j < Nw; j += nthr) {  // bias gradient: the column sums of D_l, rows in ascending order
            float g = first_sub ? 0.f : gsum[gb + j];
            for (int r = 0; r < nr; ++r) g += Dl[r * Nw + j];
            if (!last_sub) {
              gsum[gb + j] = g;
              continue;
            }
            const float w = th[gb + j];
            float mm = mg[gb + j], vv = vg[gb + j];
            if (l2b != 0.f) g = fmaf(2.f * l2b, w, g);
            th[gb + j] = adam_update(w, g, mm, vv, alpha, omb1, omb2, a.eps);
            mg[gb + j] = mm;
            vg[gb + j] = vv;
          }
        }
        __syncthreads();  // the step's theta (and the sub-tile's sums) before anybody reads them
      }
      if (L.any_l2) reg = stream_penalty(S, L, th);
    }
    if (a.epoch_loss) {
      eloss = wave_sum(eloss);  // (rows live in the first wave's slots only)
      if (tid == 0) a.epoch_loss[model * a.epochs + e] = (eloss + ereg) / (float)N;
    }
  }
  if (tid == 0) a.at[model] = t0 + (long long)a.epochs * steps;
}

}  // namespace bore

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
using namespace bore;

// Within the streamed flavour's bounds?  0, or the error (BORE_E_UNSUPPORTED names the bound); `quiet`: the code alone,
// the thread's error string left as it is.
static int stream_bounds(const bore_mlp_desc *desc, MlpLayout *L, bool quiet = false) {
  if (bore_make_layout(desc, 0, BORE_BATCH_MAX, L)) return quiet ? BORE_E_INVALID : fail(BORE_E_INVALID, "bad bore_mlp_desc");
  if (desc->compute != BORE_COMPUTE_F32) return quiet ? BORE_E_UNSUPPORTED : fail(BORE_E_UNSUPPORTED, kBf16Shapes);
  for (int l = 0; l <= L->n_layers; ++l)
    if (L->w[l] > BORE_STREAM_MAX_UNITS)
      return quiet ? BORE_E_UNSUPPORTED
                   : fail(BORE_E_UNSUPPORTED,
                          "the model does not fit one workgroup's LDS and %s %d exceeds what the streamed kernels take "
                          "(BORE_STREAM_MAX_UNITS = %d)",
                          l ? "a layer width of" : "an input dimension of", L->w[l], BORE_STREAM_MAX_UNITS);
  return 0;
}

// The same as a predicate.
static bool stream_within_bounds(const bore_mlp_desc *desc) {
  MlpLayout L;
  return stream_bounds(desc, &L, true) == 0;
}

// BORE_STREAM = 1 (tests, A/B): any float32 request within the bounds takes the streamed flavour.
static bool stream_forced(const bore_mlp_desc *desc) {
  const char *env = getenv("BORE_STREAM");
  if (!env || !atoi(env) || !desc || g_batch) return false;
  return stream_within_bounds(desc);
}

// Workgroups per model that walk its `tiles` row tiles (or groups of restarts), `ws_floats` of workspace each: with
// `cu_cap` two per CU's worth over the models, never more than there is work, never more than STREAM_WS_BYTES of
// workspace per call (one per model at least: 64 MiB is 512 at 8->256-256-1 and 32 at eight layers of 512), <= 65535.
static long long stream_walkers(int n_models, long long tiles, long long ws_floats, bool cu_cap) {
  long long gy = tiles;
  const long long cap = cu_cap ? (2 * device_cus() + n_models - 1) / n_models : gy;
  if (gy > cap) gy = cap;
  const long long by_bytes = STREAM_WS_BYTES / ((long long)n_models * ws_floats * (long long)sizeof(float));
  if (gy > by_bytes) gy = by_bytes;
  if (gy > 65535) gy = 65535;
  return gy < 1 ? 1 : gy;
}

static int stream_rows(bool with_grad, const bore_mlp_desc *desc, int n_models, const float *theta, const float *Xf,
                       const double *Xd, int64_t n_rows, int x_shared, int transform, float sign, float *out,
                       double *grad, void *stream) {
  StreamRowArgs a;
  if (const int rc = stream_bounds(desc, &a.L)) return rc;
  if (n_models < 1) return fail(BORE_E_INVALID, "n_models must be >= 1 (got %d)", n_models);
  if (a.L.w[a.L.n_layers] != 1) return fail(BORE_E_INVALID, "the last Dense layer must have 1 unit");
  if (!theta || !(with_grad ? (const void *)Xd : (const void *)Xf) || !out || (with_grad && !grad))
    return fail(BORE_E_INVALID, "null pointer");
  if (n_rows < 0) return fail(BORE_E_INVALID, "n_rows < 0");
  if (n_rows == 0) return 0;
  a.theta = theta; a.Xf = Xf; a.Xd = Xd; a.out = out; a.grad = grad;
  a.n_rows = n_rows; a.x_shared = x_shared; a.transform = transform; a.sign = sign;
  a.ws_stride = (long long)stream_tile_floats(a.L);
  const long long gy = stream_walkers(n_models, (n_rows + SROWS - 1) / SROWS, a.ws_stride, true);
  hipStream_t st = (hipStream_t)stream;
  return with_workspace((size_t)n_models * gy * a.ws_stride, stream, "streamed rows kernel", [&](float *ws) {
    a.ws = ws;
    const dim3 grid(n_models, (unsigned)gy);
    if (with_grad) hipLaunchKernelGGL(stream_rows_kernel<true>, grid, dim3(BORE_THREADS), 0, st, a);
    else hipLaunchKernelGGL(stream_rows_kernel<false>, grid, dim3(BORE_THREADS), 0, st, a);
    return 0;
  });
}

static int stream_forward_entry(const bore_mlp_desc *desc, int n_models, const float *theta, const float *X,
                                int64_t n_rows, int x_shared, float *out, void *stream) {
  return stream_rows(false, desc, n_models, theta, X, nullptr, n_rows, x_shared, 0, 1.f, out, nullptr, stream);
}

static int stream_value_and_input_grad(const bore_mlp_desc *desc, int n_models, const float *theta, const double *X,
                                       int64_t n_rows, int transform, int negate, float *val, double *grad,
                                       void *stream) {
  if (const int rc = check_transform("value_and_input_grad", transform)) return rc;
  return stream_rows(true, desc, n_models, theta, nullptr, X, n_rows, 0, transform, negate ? -1.f : 1.f, val, grad,
                     stream);
}

static int stream_evaluate(const bore_mlp_desc *desc, int n_models, const float *theta, const float *X, const float *z,
                           const float *sample_weight, int64_t N, float *loss, float *acc, void *stream) {
  StreamEvalArgs a;
  if (const int rc = stream_bounds(desc, &a.L)) return rc;
  if (n_models < 1) return fail(BORE_E_INVALID, "n_models must be >= 1 (got %d)", n_models);
  if (a.L.w[a.L.n_layers] != 1) return fail(BORE_E_INVALID, "evaluate: the last Dense layer must have 1 unit");
  if (!theta || !X || !z || !loss || !acc) return fail(BORE_E_INVALID, "evaluate: null pointer");
  if (N < 1) return fail(BORE_E_INVALID, "evaluate: N < 1");
  a.theta = theta; a.X = X; a.z = z; a.loss = loss; a.acc = acc; a.N = N;
  a.ws_stride = (long long)stream_tile_floats(a.L);
  hipStream_t st = (hipStream_t)stream;
  a.sw = sample_weight;
  return with_workspace((size_t)n_models * a.ws_stride, stream, "streamed evaluate kernel", [&](float *ws) {
    a.ws = ws;
    if (sample_weight) hipLaunchKernelGGL(stream_evaluate_kernel<true>, dim3(n_models), dim3(BORE_THREADS), 0, st, a);
    else hipLaunchKernelGGL(stream_evaluate_kernel<false>, dim3(n_models), dim3(BORE_THREADS), 0, st, a);
    return 0;
  });
}

static int stream_fit(const FitRequest &r, void *stream) {
  StreamFitArgs a;
  const int n_models = r.n_models, epochs = r.epochs, batch_size = r.batch_size;
  const int64_t N = r.N;
  if (const int rc = stream_bounds(r.desc, &a.L)) return rc;
  if (n_models < 1) return fail(BORE_E_INVALID, "n_models must be >= 1 (got %d)", n_models);
  if (batch_size < 1) return fail(BORE_E_INVALID, "fit: batch_size must be positive (got %d)", batch_size);
  if (N < 1 || N > (1 << 24)) return fail(BORE_E_INVALID, "fit: N=%lld out of range", (long long)N);
  const MlpLayout &L = a.L;
  if (const int rc = fit_check_request(L, r)) return rc < 0 ? rc : 0;
  // the call's shuffles, when the caller passes none: the project's one stream (shuffle_kernel), drawn into the
  // scratch in front of the fit on the same stream
  const size_t perm_ints = r.perm ? 0 : (size_t)n_models * epochs * N;
  // (as long as shuffle_kernel can rank N rows in LDS and the call's shuffles take no more than STREAM_WS_BYTES;
  // beyond: the caller's turn, which bore_amd.models takes a few epochs per launch)
  if (!r.perm && (epochs > 65535 || (size_t)perm_scratch_floats(N) * 4 > BORE_LDS_BYTES ||
                perm_ints * sizeof(int32_t) > (size_t)STREAM_WS_BYTES))
    return fail(BORE_E_NEEDS_PERM,
                "fit: the shuffles of %d models x %d epochs x N=%lld rows are not drawn on the device (more rows than "
                "an LDS ranks, or more than %lld MiB of them): pass explicit shuffles (`perm`, e.g. from "
                "bore_amd.shuffle.permutations) -- any N then",
                n_models, epochs, (long long)N, STREAM_WS_BYTES >> 20);
  fit_fill<false>(a, r);
  a.o_g = (long long)stream_tile_floats(L);
  a.ws_stride = a.o_g + (batch_size > BORE_BATCH_MAX ? L.P : 0);
  hipStream_t st = (hipStream_t)stream;
  const size_t ws_floats = (size_t)n_models * a.ws_stride;
  return with_workspace(ws_floats + perm_ints, stream, "streamed fit kernel", [&](float *buf) {
    a.ws = buf;
    if (!r.perm) {
      int32_t *drawn = reinterpret_cast<int32_t *>(buf + ws_floats);
      if (const int rc = bore_shuffle_perm(r.seed, r.model_index0, n_models, r.epoch0, epochs, N, drawn, stream)) return rc;
      a.perm = drawn;
    }
    a.sw = r.sample_weight;
    if (r.sample_weight) hipLaunchKernelGGL(stream_fit_kernel<true>, dim3(n_models), dim3(BORE_THREADS), 0, st, a);
    else hipLaunchKernelGGL(stream_fit_kernel<false>, dim3(n_models), dim3(BORE_THREADS), 0, st, a);
    return 0;
  });
}

extern "C" int bore_mlp_streamed(const bore_mlp_desc *desc) {
  MlpLayout L;
  if (bore_make_layout(desc, 0, BORE_BATCH_MAX, &L)) return fail(BORE_E_INVALID, "bad bore_mlp_desc");
  if (desc->compute != BORE_COMPUTE_F32) return 0;  // (bfloat16: the wide static shapes, never streamed)
  int mask = 0;
  if (check_common(desc, 1, 0, BORE_BATCH_MAX, true, BORE_BATCH_MAX + BORE_LAYOUT_FLOATS + 4, &L) == BORE_E_UNSUPPORTED)
    mask |= 1;
  if (check_common(desc, 1, 2, BORE_BATCH_MAX, true, BORE_BATCH_MAX + BORE_LAYOUT_FLOATS + 4, &L) == BORE_E_UNSUPPORTED)
    mask |= 2;
  FitPlan p;  // (the fit's own capacity check at one row and 64-row batches, outside batch mode)
  if (fit_plan(desc, 1, 1, BORE_BATCH_MAX, false, nullptr, p) == BORE_E_UNSUPPORTED && !p.fits) mask |= 4;
  g_bore_err[0] = 0;  // (a refusal above is this query's answer, not its error)
  if (mask)  // (refused by the LDS flavours: inside the streamed flavour's bounds, or the bound by name)
    if (const int rc = stream_bounds(desc, &L)) return rc;
  return mask;
}

// ---- acquisition for streamed networks: screening and restarts -------------------------------------------------------
// What the three entry points share: any float32 network within stream_bounds (one that fits LDS as well: no switch),
// never batch mode.  No HIP call.
static int stream_acq_bounds(const char *who, const bore_mlp_desc *desc, int n_models, const float *theta, MlpLayout *L) {
  if (!desc || !theta) return fail(BORE_E_INVALID, "%s: null pointer", who);
  if (n_models < 1) return fail(BORE_E_INVALID, "n_models must be >= 1 (got %d)", n_models);
  if (g_batch) return fail(BORE_E_UNSUPPORTED, "%s: batch mode (bore_set_batch) keeps the network in LDS", who);
  if (const int rc = stream_bounds(desc, L)) return rc;
  if (L->w[L->n_layers] != 1) return fail(BORE_E_INVALID, "%s: the last Dense layer must have 1 unit", who);
  return 0;
}

// What the screenings of both flavours run behind their request checks.  ONE buffer: the walkers' workspaces
// (`ws_stride` floats each, the rows kernels' geometry) and, unless the caller takes them (`pred`), the predictions;
// launch_pred(ws, out, gy) is the flavour's forward pass over the candidates; the selection is stream_select_kernel,
// which ranks a prediction buffer and never looks at the network.
template <class LaunchPred>
static int stream_screen_tail(const char *who, int n_models, int64_t n_samples, int num_starts, int D, int x_shared,
                              const double *X_init, const StreamSampleArgs &sp, long long ws_stride, double *x0,
                              int32_t *idx, float *pred, void *stream, LaunchPred launch_pred) {
  int n_pad = 1;
  while (n_pad < n_samples) n_pad <<= 1;
  // (the rule's clamp to 65535 never binds here: n_samples <= BORE_STREAM_MAX_SAMPLES = 16384 is at most 256 tiles)
  const long long gy = stream_walkers(n_models, (n_samples + SROWS - 1) / SROWS, ws_stride, true);
  const size_t ws_floats = (size_t)n_models * gy * ws_stride;
  const size_t pred_floats = pred ? 0 : (size_t)n_models * n_samples;
  return with_workspace(ws_floats + pred_floats, stream, who, [&](float *buf) {
    float *out = pred ? pred : buf + ws_floats;
    StreamSelectArgs sel;
    sel.X = X_init; sel.pred = out; sel.x0 = x0; sel.idx = idx;
    sel.n_samples = n_samples; sel.x_shared = x_shared; sel.R = num_starts; sel.n_pad = n_pad; sel.D = D;
    const size_t key_bytes = 8 * ((size_t)n_pad + 32) + 8;
    if (const int rc = allow_lds(stream_select_kernel, key_bytes)) return rc;
    launch_pred(buf, out, gy);
    hipLaunchKernelGGL(stream_select_kernel, dim3(n_models), dim3(BORE_THREADS), key_bytes, (hipStream_t)stream, sel, sp);
    return 0;
  });
}

// What the restart entry points of both flavours run behind their request checks, a.r filled but for the geometry:
// the carve (stream_restart.h) beside `static_bytes` of the kernel's static LDS, the grid, the round cap, the launch
// around a workspace of `ws_stride` floats per workgroup.
template <class K, class Args>
static int stream_restart_launch(const char *who, const char *what, K kernel, Args &a, int D, size_t static_bytes,
                                 int n_models, long long ws_stride, const bore_lbfgsb_opts *opts, void *stream) {
  static_assert(STREAM_RESTART_LDS_BYTES == BORE_LDS_BYTES, "stream_restart.h carves another LDS");
  RestartArgs &r = a.r;
  RestartCarve c;
  if (!stream_restart_carve(D, r.opt.m, static_bytes, BORE_THREADS / 64, &c))
    return fail(BORE_E_UNSUPPORTED,
                "%s: one problem's workspace (%zu B at D = %d, maxcor = %d) does not fit the %zu B of LDS beside the "
                "streamed kernels' panels: lower maxcor", who, (size_t)c.lds.prob_floats * 4, D, r.opt.m, c.room);
  r.lds = c.lds;
  r.waves = c.waves;
  // a model's restarts in groups of `waves`, a workgroup per group -- fewer, each walking several groups, when the
  // workspaces of all would take more than STREAM_WS_BYTES
  r.ws_stride = ws_stride;
  const long long groups = ((long long)r.R + c.waves - 1) / c.waves;
  const long long gy = stream_walkers(n_models, groups, ws_stride, false);  // (the restarts take no CU cap)
  // every round serves one request of every live problem: a wave's problems, one after another, each within the
  // optimiser's own limit (lbfgsb_round_cap)
  r.max_rounds = ((groups + gy - 1) / gy) * lbfgsb_round_cap(opts);
  if (const int rc = allow_lds(kernel, c.lds_bytes)) return rc;
  return with_workspace((size_t)n_models * gy * ws_stride, stream, what, [&](float *ws) {
    r.ws = ws;
    hipLaunchKernelGGL(kernel, dim3(n_models, (unsigned)gy), dim3(BORE_THREADS), c.lds_bytes, (hipStream_t)stream, a);
    return 0;
  });
}

static int stream_screen(const char *who, const bore_mlp_desc *desc, int n_models, const float *theta,
                         const double *X_init, const SampleSpec *spec, int64_t n_samples, int x_shared, int num_starts,
                         double *x0, int32_t *idx, float *pred, void *stream) {
  StreamRowArgs a;
  if (const int rc = stream_acq_bounds(who, desc, n_models, theta, &a.L)) return rc;
  const int D = a.L.w[0];
  if (spec && D > BORE_DIM_MAX)
    return fail(BORE_E_UNSUPPORTED, "%s: the sampled form takes D <= BORE_DIM_MAX = %d (got %d)", who, BORE_DIM_MAX, D);
  if ((!X_init && !spec) || !x0 || !idx || (spec && (!spec->low || !spec->high)))
    return fail(BORE_E_INVALID, "%s: null pointer", who);
  if (n_samples < 1) return fail(BORE_E_INVALID, "%s: n_samples out of range", who);
  if (num_starts < 1 || num_starts > n_samples)
    return fail(BORE_E_INVALID, "%s: need 1 <= num_starts <= n_samples", who);
  if (n_samples > BORE_STREAM_MAX_SAMPLES)
    return fail(BORE_E_UNSUPPORTED,
                "%s: the selection ranks n_samples <= BORE_STREAM_MAX_SAMPLES = %d sort keys in one workgroup's LDS "
                "(got %lld)", who, BORE_STREAM_MAX_SAMPLES, (long long)n_samples);
  StreamSampleArgs sp;
  sp.sampled = spec != nullptr;
  sp.seed = 0; sp.model0 = 0; sp.draw = 0;
  if (spec) {
    sp.seed = spec->seed; sp.model0 = spec->model_index0; sp.draw = spec->draw_index;
    for (int d = 0; d < D; ++d) {
      sp.box.lo[d] = spec->low[d];
      sp.box.hi[d] = spec->high[d];
    }
  }
  // the predictions: the rows kernel's geometry (stream_rows)
  a.theta = theta; a.Xf = nullptr; a.Xd = X_init; a.grad = nullptr;
  a.n_rows = n_samples; a.x_shared = x_shared; a.transform = 0; a.sign = 1.f;
  a.ws_stride = (long long)stream_tile_floats(a.L);
  return stream_screen_tail(who, n_models, n_samples, num_starts, D, x_shared, X_init, sp, a.ws_stride, x0, idx, pred,
                            stream, [&](float *ws, float *out, long long gy) {
                              a.ws = ws;
                              a.out = out;
                              hipLaunchKernelGGL(stream_screen_pred_kernel, dim3(n_models, (unsigned)gy),
                                                 dim3(BORE_THREADS), 0, (hipStream_t)stream, a, sp);
                            });
}

extern "C" int bore_stream_screen_topk(const bore_mlp_desc *desc, int n_models, const float *theta,
                                       const double *X_init, int64_t n_samples, int x_shared, int num_starts,
                                       double *x0, int32_t *idx, float *pred, void *stream) {
  if (!X_init) return fail(BORE_E_INVALID, "stream_screen_topk: null pointer");
  return stream_screen("stream_screen_topk", desc, n_models, theta, X_init, nullptr, n_samples, x_shared, num_starts,
                       x0, idx, pred, stream);
}

extern "C" int bore_stream_sample_screen_topk(const bore_mlp_desc *desc, int n_models, const float *theta, uint64_t seed,
                                              int64_t model_index0, int64_t draw_index, int64_t n_samples,
                                              const double *low, const double *high, int num_starts, double *x0,
                                              int32_t *idx, float *pred, void *stream) {
  const SampleSpec spec{seed, model_index0, draw_index, low, high};
  return stream_screen("stream_sample_screen_topk", desc, n_models, theta, nullptr, &spec, n_samples, 0, num_starts, x0,
                       idx, pred, stream);
}

extern "C" int bore_stream_lbfgsb_minimize(const bore_mlp_desc *desc, int n_models, const float *theta, int transform,
                                           int negate, const double *x0, int num_starts, const double *lb,
                                           const double *ub, const bore_lbfgsb_opts *opts, double *x, double *fun,
                                           double *jac, int32_t *info, void *stream) {
  static const char who[] = "stream_lbfgsb_minimize";
  StreamLbfgsbArgs a;
  if (const int rc = stream_acq_bounds(who, desc, n_models, theta, &a.L)) return rc;
  const int D = a.L.w[0];
  if (D > BORE_DIM_MAX)
    return fail(BORE_E_UNSUPPORTED, "%s: the restarts take D <= BORE_DIM_MAX = %d (got %d)", who, BORE_DIM_MAX, D);
  if (const int rc = lbfgsb_check_args(LbfgsbRequest{desc, n_models, theta, transform, negate, x0, num_starts, lb, ub, opts,
                                                     x, fun, jac, info}, a.r.box, a.r.nbd, a.r.opt))
    return rc;
  a.theta = theta; a.r.x0 = x0; a.r.x = x; a.r.fun = fun; a.r.jac = jac; a.r.info = info;
  a.r.R = num_starts; a.r.transform = transform; a.r.sign = negate ? -1.f : 1.f;
  // (static LDS: the panels; per workgroup one workspace tile)
  return stream_restart_launch(who, "streamed restart kernel", stream_lbfgsb_kernel, a, D, sizeof(StreamLds), n_models,
                               (long long)stream_tile_floats(a.L), opts, stream);
}

extern "C" int bore_stream_svgd_optimize(const bore_mlp_desc *desc, int n_models, const float *theta, int transform,
                                         const double *x_init, int n_particles, const double *lb, const double *ub,
                                         const bore_svgd_opts *opts, double *x_out, void *stream) {
  static const char who[] = "stream_svgd_optimize";
  StreamSvgdArgs a;
  if (!x_init || !x_out || !opts) return fail(BORE_E_INVALID, "%s: null pointer", who);
  if (const int rc = stream_acq_bounds(who, desc, n_models, theta, &a.L)) return rc;
  const int D = a.L.w[0], n = n_particles;
  if (D > BORE_DIM_MAX)
    return fail(BORE_E_UNSUPPORTED, "%s: the box goes by value, D <= BORE_DIM_MAX = %d (got %d)", who, BORE_DIM_MAX, D);
  if (n < 1 || n > BORE_SVGD_MAX_PARTICLES)  // (what fits is decided by the LDS check below: 32 n D bytes of state)
    return fail(BORE_E_UNSUPPORTED, "%s: 1..%d particles per launch (got %d)", who, BORE_SVGD_MAX_PARTICLES, n);
  if (const int rc = check_transform(who, transform)) return rc;
  if (opts->n_iter < 0 || (opts->distortion != 0 && opts->distortion != 1))
    return fail(BORE_E_INVALID, "%s: bad options", who);
  if ((lb == nullptr) != (ub == nullptr)) return fail(BORE_E_INVALID, "%s: lb and ub go together", who);
  // dynamic LDS beside the static StreamLds: svgd_big_kernel's particle state, no theta, no activation tile
  const size_t nD2 = 2 * (((size_t)n * D + 1) & ~(size_t)1);  // floats of an [n][D] fp64 array, 16-B multiple
  size_t off = 0;
  a.o_x = (int)off; off += nD2;
  a.o_fg = (int)off; off += nD2;
  a.o_grad = (int)off; off += nD2;
  a.o_hist = (int)off; off += nD2;
  a.o_f = (int)off; off += 4 * (size_t)n;
  a.o_sel = (int)off; off += SVGD_SELECT_WORDS;
  const size_t lds_bytes = off * 4 + 16;  // (16: what the kernel may skip to align the dynamic region)
  // (64: the static region's own alignment, as for the restarts)
  if (sizeof(StreamLds) + 64 + lds_bytes > (size_t)BORE_LDS_BYTES)
    return fail(BORE_E_UNSUPPORTED,
                "%s: %d particles in %d dimensions need %zu B of LDS (> %d) beside the streamed kernels' panels: the "
                "particle state is 32 n D bytes",
                who, n, D, sizeof(StreamLds) + 64 + lds_bytes, BORE_LDS_BYTES);
  // one workspace tile per model, never walked: a second geometry would be a second, untested code path
  a.ws_stride = (long long)stream_tile_floats(a.L);
  if ((long long)n_models * a.ws_stride * (long long)sizeof(float) > STREAM_WS_BYTES)
    return fail(BORE_E_UNSUPPORTED,
                "%s: %d models x one %lld B workspace tile exceed the %lld MiB a streamed call allows itself "
                "(STREAM_WS_BYTES): fewer models per call",
                who, n_models, a.ws_stride * (long long)sizeof(float), STREAM_WS_BYTES >> 20);
  a.clip = lb != nullptr;
  for (int d = 0; d < BORE_DIM_MAX; ++d) {
    a.lo[d] = lb && d < D ? lb[d] : 0.0;
    a.hi[d] = ub && d < D ? ub[d] : 0.0;
  }
  a.theta = theta; a.x_init = x_init; a.x_out = x_out;
  a.n = n; a.n_iter = opts->n_iter; a.transform = transform; a.distortion = opts->distortion;
  a.step = opts->step_size; a.alpha = opts->alpha; a.eps = opts->eps; a.tau = opts->tau;
  a.length_scale = opts->length_scale; a.dparam = opts->distortion_param;
  if (const int rc = allow_lds(stream_svgd_kernel, lds_bytes)) return rc;
  return with_workspace((size_t)n_models * a.ws_stride, stream, "streamed SVGD kernel", [&](float *ws) {
    a.ws = ws;
    hipLaunchKernelGGL(stream_svgd_kernel, dim3(n_models), dim3(BORE_THREADS), lds_bytes, (hipStream_t)stream, a);
    return 0;
  });
}
