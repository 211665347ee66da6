// bore_lstm_stream.hip -- the STREAMED flavour of the multi-fidelity classifier (bore_lstm.hip): recurrent
// networks whose parameters and one tile of state do not fit one workgroup's LDS.  Entry points of its own,
// bore_lstm_stream_forward / _value_and_input_grad / _fit / _evaluate, the host query bore_lstm_streamed and, for
// the acquisition of the one-to-one network, bore_lstm_stream_screen_topk / _lbfgsb_minimize (include/bore_hip.h);
// bore_lstm_* keep their kernels, their refusals and their bits.  Included from bore_all.hip after bore_stream.hip,
// whose stream_gemm forms every matrix product here and whose stream_select_kernel ranks the screening's predictions.
//
// theta stays in global memory.  A workgroup of BORE_THREADS takes a tile of up to 64 sequences; everything the
// tile needs lives in a stream-ordered device workspace (hipMallocAsync), rows packed at the tile's row count:
//   XH_l [step][row][in_l + H + 1]   the input of cell l at a step, the cell's h of the step before, and a 1
//   HT   [step][row][H + 1]          the top cell's h at a step, and a 1 (the head's input)
//   gates, c, the gate deltas dZ_l [step][row][4H], the mask, logits and their deltas [step][row]
// (the 1 columns and the per-step copies only where a backward pass reads them: the forward-only kernels keep
// one step).  W_l, U_l and b_l are adjacent in the packed vector, rows of 4H floats each, so [W_l; U_l; b_l] is
// ONE (in_l + H + 1) x 4H matrix and per (step, cell)
//   Z = b_l + [x | h'] [W_l; U_l]              one stream_gemm, the bias through `init`
//   d[x | h'] = dZ [W_l; U_l]^T                one stream_gemm with the transposed operand
// and, after the whole backward pass of an Adam step,
//   d[W_l; U_l; b_l] = XH_l^T dZ_l             one stream_gemm whose reduction runs over (step, row)
// with the Adam update in its epilogue (the head the same way from HT and the logit deltas).  Every output element
// of stream_gemm is one fmaf chain in ascending order of the reduction index, so a gradient does not depend on the
// run, on n_models or on the tiles of a launch; a row alone gives the bits it gives in a full tile, a model alone
// the bits of a multi-model launch.  The gate non-linearities and the c / h update are an elementwise phase over
// (sequence, unit) items between the products; a masked step is a select.  No float atomics; data crosses waves
// of ONE workgroup through the workspace around __syncthreads() (bore_stream.hip's hand-over rule); no workgroup
// waits for another one -- evaluate's tiles leave partial sums that a second small kernel adds in tile order.
//
// The scalar arithmetic is the LDS flavour's, each formula defined once: the cell and the masked loss in lstm_math.h
// (all but the line that forms c: see tile_forward), objective_transform, adam_update_ieee and AdamClock in
// mlp_math.h, step_live and l2_of in bore_lstm.hip, which also holds the request checks of both flavours.

namespace bore_lstm_stream {

using bore::StreamLds, bore::stream_gemm, bore::stream_wg_sum, bore::objective_transform;
using bore::AdamClock, bore::adam_update_ieee;
using bore_lstm::Lay, bore_lstm::Src, bore_lstm::l2_of, bore_lstm::step_live;
using bore_lstm::Gates, bore_lstm::gates_of, bore_lstm::cell_out, bore_lstm::GateDeltas, bore_lstm::gate_deltas;
using bore_lstm::masked_bce, bore_lstm::masked_hit, bore_lstm::l2_term;

constexpr int ROWS = bore::SROWS;  // sequences per tile (batch_size <= 64)
constexpr int MAXL = BORE_LSTM_MAX_LAYERS;
constexpr int NTH = BORE_THREADS;
static_assert(ROWS == bore_lstm::TILE, "both flavours tile 64 sequences");

enum WsMode { WS_FORWARD = 0, WS_VALUE_GRAD = 1, WS_FIT = 2 };

struct SLay {
  Lay a;               // the network and its packed offsets (the LDS offsets of Lay are not used here)
  int keep, keep_dz;   // every step's activations / gate deltas stay in the workspace (else: the current step's only)
  long long o_xh[MAXL], o_ht, o_gate, o_c, o_mask, o_logit, o_dlogit, o_dz, o_dhc, o_dcc, o_din, o_dx;
  long long ws_floats;  // of one tile
};

// --------------------------------------------------------------------------------------------------
// host: descriptor -> bounds, workspace layout
// --------------------------------------------------------------------------------------------------
static int stream_lay(const bore_lstm_desc *d, int T, int mode, SLay *y) {
  if (const int rc = bore_lstm::lay_packed(d, T, "lstm_stream", BORE_LSTM_STREAM_MAX_INPUT, "BORE_LSTM_STREAM_MAX_INPUT",
                                           BORE_LSTM_STREAM_MAX_UNITS, "BORE_LSTM_STREAM_MAX_UNITS", y->a))
    return rc;
  const Lay &a = y->a;
  y->keep = mode != WS_FORWARD;
  y->keep_dz = mode == WS_FIT;
  long long s = 0;
  auto take = [&s](long long n) {
    const long long o = s;
    s += (n + 3) & ~3LL;
    return o;
  };
  const long long tile = ROWS, sl = y->keep ? a.T : 1;
  for (int l = 0; l < a.L; ++l) y->o_xh[l] = take(sl * tile * (a.in_dim[l] + a.H + 1));
  y->o_ht = take(sl * tile * (a.H + 1));
  y->o_gate = take(a.L * sl * tile * a.G);
  y->o_c = take(a.L * sl * tile * a.H);
  y->o_mask = take(a.T * tile);
  y->o_logit = take(a.T * tile);
  y->o_dlogit = take(a.T * tile);
  y->o_dz = y->o_dhc = y->o_dcc = y->o_din = y->o_dx = 0;
  if (mode != WS_FORWARD) {
    y->o_dz = take((mode == WS_FIT ? (long long)a.L * a.T : 1) * tile * a.G);
    y->o_dhc = take(a.L * tile * a.H);
    y->o_dcc = take(a.L * tile * a.H);
    y->o_din = take(tile * a.H);
    y->o_dx = take(tile * a.D);
  }
  y->ws_floats = s;
  return 0;
}

// --------------------------------------------------------------------------------------------------
// device
// --------------------------------------------------------------------------------------------------
__device__ __forceinline__ int k1_of(const Lay &a, int l) { return a.in_dim[l] + a.H + 1; }
// XH_l / HT / gates / c of step t (without keep: of the one step there is); nr rows per step
__device__ __forceinline__ float *xh_at(const SLay &y, float *ws, int l, int t, int nr) {
  return ws + y.o_xh[l] + (long long)(y.keep ? t : 0) * nr * k1_of(y.a, l);
}
__device__ __forceinline__ float *ht_at(const SLay &y, float *ws, int t, int nr) {
  return ws + y.o_ht + (long long)(y.keep ? t : 0) * nr * (y.a.H + 1);
}
__device__ __forceinline__ float *gate_at(const SLay &y, float *ws, int l, int t, int nr) {
  return ws + y.o_gate + (y.keep ? ((long long)l * y.a.T * ROWS + (long long)t * nr) * y.a.G : (long long)l * ROWS * y.a.G);
}
__device__ __forceinline__ float *c_at(const SLay &y, float *ws, int l, int t, int nr) {
  return ws + y.o_c + (y.keep ? ((long long)l * y.a.T * ROWS + (long long)t * nr) * y.a.H : (long long)l * ROWS * y.a.H);
}
__device__ __forceinline__ float *dz_at(const SLay &y, float *ws, int l, int t, int nr) {
  return ws + y.o_dz + (y.keep_dz ? ((long long)l * y.a.T * ROWS + (long long)t * nr) * y.a.G : 0);
}

// What a tile needs before its first step: the mask [t][b]; with a backward pass ahead, the 1 columns; and h = 0
// in front of step 0.  Ends with a barrier.
template <typename XT>
__device__ __forceinline__ void tile_begin(const SLay &y, float *ws, const Src<XT> &src, const int *rows, int nr, int T,
                                           int use_mask, float mask_value) {
  const Lay &a = y.a;
  const int tid = threadIdx.x, H = a.H;
  float *mask = ws + y.o_mask;
  for (int it = tid; it < nr * T; it += NTH) {
    const int t = it / nr, b = it - t * nr;
    mask[it] = step_live(a, src, rows, b, t, use_mask, mask_value) ? 1.f : 0.f;
  }
  for (int l = 0; l < a.L; ++l) {
    const int K1 = k1_of(a, l), in = a.in_dim[l];
    float *x0 = xh_at(y, ws, l, 0, nr);
    for (int it = tid; it < nr * H; it += NTH) x0[(it / H) * K1 + in + it % H] = 0.f;
    if (y.keep_dz)
      for (int it = tid; it < nr * T; it += NTH) x0[it * K1 + K1 - 1] = 1.f;
  }
  if (y.keep_dz) {
    float *h0 = ht_at(y, ws, 0, nr);
    for (int it = tid; it < nr * T; it += NTH) h0[it * (H + 1) + H] = 1.f;
  }
  __syncthreads();
}

// Forward pass of one tile over T steps: logits [t][b] in the workspace; with y.keep the activations of every
// step stay behind for the backward pass.  Called by the whole workgroup after tile_begin; ends with a barrier.
template <typename XT>
__device__ __forceinline__ void tile_forward(StreamLds &S, const SLay &y, const float *th, float *ws, const Src<XT> &src,
                                             const int *rows, int nr, int T) {
  const Lay &a = y.a;
  const int tid = threadIdx.x, H = a.H, G = a.G, L = a.L, D = a.D;
  const bool keep = y.keep != 0;
  const float *mask = ws + y.o_mask;
  float *logit = ws + y.o_logit;
  for (int t = 0; t < T; ++t) {
    {  // the step's inputs into XH_0
      float *x0 = xh_at(y, ws, 0, t, nr);
      const int K1 = k1_of(a, 0);
      for (int it = tid; it < nr * D; it += NTH) {
        const int b = it / D, k = it - b * D;
        x0[b * K1 + k] = src.x(rows, b, t, k);
      }
    }
    __syncthreads();
    for (int l = 0; l < L; ++l) {
      const int in = a.in_dim[l], K1 = in + H + 1;
      float *xh = xh_at(y, ws, l, t, nr), *Z = gate_at(y, ws, l, t, nr);
      const float *bias = th + a.gb[l];
      stream_gemm<false, false>(
          S, nr, G, in + H, xh, K1, th + a.gW[l], G, [&](int, const int j) { return bias[j]; },
          [&](const int i, const int j, const float v) { Z[i * G + j] = v; });
      // the gates of (sequence, unit) items; h goes to this cell's next step and to the cell above (or the head)
      float *cc = c_at(y, ws, l, t, nr);
      const float *cpv = t > 0 ? c_at(y, ws, l, t - 1, nr) : nullptr;
      float *hnext = (!keep || t + 1 < T) ? xh_at(y, ws, l, t + 1, nr) : nullptr;
      float *up = l + 1 < L ? xh_at(y, ws, l + 1, t, nr) : ht_at(y, ws, t, nr);
      const int upK = l + 1 < L ? 2 * H + 1 : H + 1;
      for (int it = tid; it < nr * H; it += NTH) {
        const int b = it / H, u = it - b * H;
        float *z = Z + b * G;
        const Gates g = gates_of(a.act, z[u], z[H + u], z[2 * H + u], z[3 * H + u]);
        const float cp = cpv ? cpv[it] : 0.f;
        // one product and an fmaf, two roundings; the LDS flavour forms f * cp + i * g, three
        const float c = fmaf(g.f, cp, g.i * g.g);
        float cn, hn;
        cell_out(a.act, g.o, c, cp, xh[b * K1 + in + u], mask[t * nr + b] != 0.f, cn, hn);
        if (keep) {
          z[u] = g.i; z[H + u] = g.f; z[2 * H + u] = g.g; z[3 * H + u] = g.o;
        }
        cc[it] = cn;
        if (hnext) hnext[b * K1 + in + u] = hn;
        up[b * upK + u] = hn;
      }
      __syncthreads();
    }
    // Dense head on the top cell's output
    const float *ht = ht_at(y, ws, t, nr);
    const float bo = th[a.gbo];
    stream_gemm<false, false>(
        S, nr, 1, H, ht, H + 1, th + a.gWo, 1, [&](int, int) { return bo; },
        [&](const int i, int, const float v) { logit[t * nr + i] = v; });
  }
}

// Backpropagation through time of one tile from dlogit [t][b]: the gate deltas (every step's with y.keep_dz),
// and with want_dx dx [b][k] = d/dx summed over the steps.  Reads theta, writes none of it.
__device__ __forceinline__ void tile_backward(StreamLds &S, const SLay &y, const float *th, float *ws, int nr, int T,
                                              bool want_dx) {
  const Lay &a = y.a;
  const int tid = threadIdx.x, H = a.H, G = a.G, L = a.L, D = a.D;
  const float *mask = ws + y.o_mask, *dlogit = ws + y.o_dlogit, *Wo = th + a.gWo;
  float *din = ws + y.o_din, *dx = ws + y.o_dx;
  for (int i = tid; i < L * ROWS * H; i += NTH) ws[y.o_dhc + i] = ws[y.o_dcc + i] = 0.f;
  if (want_dx)
    for (int i = tid; i < nr * D; i += NTH) dx[i] = 0.f;
  __syncthreads();
  for (int t = T - 1; t >= 0; --t) {
    for (int l = L - 1; l >= 0; --l) {
      const int in = a.in_dim[l];
      float *dhl = ws + y.o_dhc + (long long)l * ROWS * H, *dcl = ws + y.o_dcc + (long long)l * ROWS * H;
      float *dz = dz_at(y, ws, l, t, nr);
      const float *gts = gate_at(y, ws, l, t, nr), *ct = c_at(y, ws, l, t, nr);
      const float *cpv = t > 0 ? c_at(y, ws, l, t - 1, nr) : nullptr;
      for (int it = tid; it < nr * H; it += NTH) {
        const int b = it / H, u = it - b * H;
        const float above = l == L - 1 ? dlogit[t * nr + b] * Wo[u] : din[it];
        const float dh = dhl[it] + above;
        const float *g = gts + b * G;
        const GateDeltas dl = gate_deltas(a.act, Gates{g[u], g[H + u], g[2 * H + u], g[3 * H + u]}, ct[it],
                                          cpv ? cpv[it] : 0.f, dh, dcl[it], mask[t * nr + b] != 0.f);
        float *d = dz + b * G;
        d[u] = dl.zi; d[H + u] = dl.zf; d[2 * H + u] = dl.zg; d[3 * H + u] = dl.zo;
        dcl[it] = dl.c;
        dhl[it] = dh;  // (a masked step passes h's gradient to the step before; a live one: replaced below)
      }
      __syncthreads();
      // d[x | h'] = dZ [W; U]^T: columns below `in` are the delta of the cell below (or of the inputs), the rest
      // the recurrent delta of the live rows.  Without a consumer the x columns are not formed.
      const int c0 = (l > 0 || want_dx) ? 0 : in;
      stream_gemm<false, true>(
          S, nr, in + H - c0, G, dz, G, th + a.gW[l] + c0 * G, G, [](int, int) { return 0.f; },
          [&](const int i, const int jj, const float v) {
            const int j = jj + c0;
            if (j < in) {
              if (l > 0) din[i * H + j] = v;
              else dx[i * D + j] += v;
            } else {
              float *p = dhl + i * H + (j - in);
              *p = mask[t * nr + i] != 0.f ? v : *p;
            }
          });
    }
  }
}

// BCE from the logits of one tile (bce_loss weighted by the mask); with `scale` != 0 also
// dlogit = mask (sigmoid(a) - y) scale.  Returns the weighted sum of the element losses.
__device__ __forceinline__ float tile_bce(StreamLds &S, const SLay &y, float *ws, const float *Y, const int *rows, int nr,
                                          int T, float scale) {
  const float *mask = ws + y.o_mask, *logit = ws + y.o_logit;
  float *dlogit = ws + y.o_dlogit;
  float part = 0.f;
  for (int it = threadIdx.x; it < nr * T; it += NTH) {
    const int t = it / nr, b = it - t * nr;
    const float x = logit[it], yy = Y[(long long)rows[b] * T + t];
    float d;
    part += masked_bce(x, yy, mask[it] != 0.f, scale, d);
    if (scale != 0.f) dlogit[it] = d;
  }
  return stream_wg_sum(S, part);
}

// sum of l2 factor x w^2 over the packed vector (never U: l2_of); every work-item gets it
__device__ __forceinline__ float tile_penalty(StreamLds &S, const Lay &a, const float *th) {
  float pen = 0.f;
  for (int p = threadIdx.x; p < a.P; p += NTH) pen = l2_term(l2_of(a, p), th[p], pen);
  return stream_wg_sum(S, pen);
}

__device__ __forceinline__ bool any_l2(const Lay &a) {
  bool any = false;
  for (int l = 0; l <= a.L; ++l) any |= a.l2k[l] != 0.f || a.l2b[l] != 0.f;
  return any;
}

// --------------------------------------------------------------------------------------------------
// kernels
// --------------------------------------------------------------------------------------------------
struct SFwdArgs {
  SLay y;
  const float *theta, *X;
  long long n;
  int T, m2m, use_mask;
  float mask_value;
  float *out, *ws;
};

// grid (models, tile walkers): a workgroup takes tiles blockIdx.y, blockIdx.y + gridDim.y, ...
__global__ void __launch_bounds__(NTH) lstm_stream_forward_kernel(const SFwdArgs A) {
  __shared__ StreamLds S;
  __shared__ int rows[ROWS];
  const SLay &y = A.y;
  const Lay &a = y.a;
  const int tid = threadIdx.x, T = A.T;
  const long long m = blockIdx.x;
  const float *th = A.theta + m * a.P;
  float *ws = A.ws + (m * gridDim.y + blockIdx.y) * y.ws_floats;
  const long long n_tiles = (A.n + ROWS - 1) / ROWS;
  const long long stride = A.m2m ? (long long)T * a.D : a.D;
  for (long long tile = blockIdx.y; tile < n_tiles; tile += gridDim.y) {
    const long long r0 = tile * ROWS;
    const int nr = (int)min((long long)ROWS, A.n - r0);
    for (int b = tid; b < ROWS; b += NTH) rows[b] = b < nr ? b : 0;
    Src<float> src;
    src.X = A.X + (m * A.n + r0) * stride;
    src.row_stride = stride;
    src.x_step = A.m2m ? a.D : 0;
    __syncthreads();
    tile_begin(y, ws, src, rows, nr, T, A.use_mask, A.mask_value);
    tile_forward(S, y, th, ws, src, rows, nr, T);
    const float *logit = ws + y.o_logit;
    if (A.m2m) {
      float *o = A.out + (m * A.n + r0) * T;
      for (int i = tid; i < nr * T; i += NTH) o[i] = logit[(i % T) * nr + i / T];
    } else {
      float *o = A.out + m * A.n + r0;
      for (int b = tid; b < nr; b += NTH) o[b] = logit[(T - 1) * nr + b];
    }
    __syncthreads();  // (the next tile overwrites the workspace and the rows)
  }
}

struct SVgArgs {
  SLay y;
  const float *theta;
  const double *X;
  long long n;
  int T, transform;
  float sign;
  float *val, *ws;
  double *grad;
};

// Value and input gradient of transform(sign f(x)) for the nr fp64 points of one tile (src.x rounds them to fp32:
// Keras autocast), f the one-to-one network over T steps: the value of row b goes to put_val(b, value), the gradient
// stays behind as dx [b][k] at ws + y.o_dx.  ONE definition for the rows kernel and the restarts, so the optimiser on
// the device sees the f and g bore_lstm_stream_value_and_input_grad hands the host.  Called by the whole workgroup
// with rows[] set and a barrier behind it; ends with a barrier.
template <typename PutVal>
__device__ __forceinline__ void tile_value_grad(StreamLds &S, const SLay &y, const float *th, float *ws,
                                                const Src<double> &src, const int *rows, int nr, int T, int transform,
                                                float sign, PutVal put_val) {
  tile_begin(y, ws, src, rows, nr, T, 0, 0.f);
  tile_forward(S, y, th, ws, src, rows, nr, T);
  // value and d value / d f at the last step
  const float *logit = ws + y.o_logit;
  float *dlogit = ws + y.o_dlogit;
  for (int i = threadIdx.x; i < nr * T; i += NTH) {
    const int t = i / nr, b = i - t * nr;
    float dv = 0.f;
    if (t == T - 1) {
      float v, dT;
      objective_transform(transform, sign * logit[i], v, dT);
      put_val(b, v);
      dv = sign * dT;
    }
    dlogit[i] = dv;
  }
  __syncthreads();
  tile_backward(S, y, th, ws, nr, T, true);
}

__global__ void __launch_bounds__(NTH) lstm_stream_value_grad_kernel(const SVgArgs A) {
  __shared__ StreamLds S;
  __shared__ int rows[ROWS];
  const SLay &y = A.y;
  const Lay &a = y.a;
  const int tid = threadIdx.x, T = A.T;
  const long long m = blockIdx.x;
  const float *th = A.theta + m * a.P;
  float *ws = A.ws + (m * gridDim.y + blockIdx.y) * y.ws_floats;
  const long long n_tiles = (A.n + ROWS - 1) / ROWS;
  for (long long tile = blockIdx.y; tile < n_tiles; tile += gridDim.y) {
    const long long r0 = tile * ROWS;
    const int nr = (int)min((long long)ROWS, A.n - r0);
    for (int b = tid; b < ROWS; b += NTH) rows[b] = b < nr ? b : 0;
    Src<double> src;
    src.X = A.X + (m * A.n + r0) * a.D;
    src.row_stride = a.D;
    src.x_step = 0;
    __syncthreads();
    float *val = A.val + m * A.n + r0;
    tile_value_grad(S, y, th, ws, src, rows, nr, T, A.transform, A.sign, [&](const int b, const float v) { val[b] = v; });
    const float *dx = ws + y.o_dx;
    double *g = A.grad + (m * A.n + r0) * a.D;
    for (int i = tid; i < nr * a.D; i += NTH) g[i] = (double)dx[i];
    __syncthreads();
  }
}

// --------------------------------------------------------------------------------------------------
// acquisition: screening and L-BFGS-B restarts (the twins of bore_stream.hip's stream_screen_pred_kernel and
// stream_lbfgsb_kernel; the selection stage is that file's stream_select_kernel itself, which never looks at the
// network)
// --------------------------------------------------------------------------------------------------
struct SScreenArgs {
  SLay y;
  const float *theta;
  const double *X;  // [models][n][D], or one shared [n][D]
  long long n;
  int T, x_shared;
  float *out, *ws;
};

// lstm_stream_forward_kernel's one-to-one form (its geometry and workspace) with the step's inputs read from the
// fp64 candidates.
__global__ void __launch_bounds__(NTH) lstm_stream_screen_pred_kernel(const SScreenArgs A) {
  __shared__ StreamLds S;
  __shared__ int rows[ROWS];
  const SLay &y = A.y;
  const Lay &a = y.a;
  const int tid = threadIdx.x, T = A.T;
  const long long m = blockIdx.x;
  const float *th = A.theta + m * a.P;
  float *ws = A.ws + (m * gridDim.y + blockIdx.y) * y.ws_floats;
  const long long n_tiles = (A.n + ROWS - 1) / ROWS;
  for (long long tile = blockIdx.y; tile < n_tiles; tile += gridDim.y) {
    const long long r0 = tile * ROWS;
    const int nr = (int)min((long long)ROWS, A.n - r0);
    for (int b = tid; b < ROWS; b += NTH) rows[b] = b < nr ? b : 0;
    Src<double> src;  // (src.x rounds to fp32: Keras autocast)
    src.X = A.X + ((A.x_shared ? 0 : m * A.n) + r0) * a.D;
    src.row_stride = a.D;
    src.x_step = 0;
    __syncthreads();
    tile_begin(y, ws, src, rows, nr, T, 0, 0.f);
    tile_forward(S, y, th, ws, src, rows, nr, T);
    const float *logit = ws + y.o_logit;
    float *o = A.out + m * A.n + r0;
    for (int b = tid; b < nr; b += NTH) o[b] = logit[(T - 1) * nr + b];
    __syncthreads();  // (the next tile overwrites the workspace and the rows)
  }
}

// Restarts: bore_stream.hip's stream_restart_drive (the scheme is told there) around tile_value_grad.  This flavour
// plugs in: the points as fp64 rows of a buffer behind the tile's workspace (tile_begin rounds them to fp32), ONE
// tile_value_grad over the `waves` rows, f from the values behind the points and g from the tile's dx.
struct SLbfgsbArgs {
  SLay y;
  const float *theta;
  bore::RestartArgs r;  // (ws_stride: the tile's workspace | fp64 points [4][D] | values [4])
  int T;
};

constexpr int LB_WAVES = NTH / 64;

__global__ void __launch_bounds__(NTH) lstm_stream_lbfgsb_kernel(const SLbfgsbArgs a) {
  __shared__ StreamLds S;
  __shared__ int rows[ROWS];
  const SLay &y = a.y;
  const long long model = blockIdx.x;
  const int D = y.a.D, NW = a.r.waves;
  const float *th = a.theta + model * y.a.P;
  float *ws = a.r.ws + (model * gridDim.y + blockIdx.y) * a.r.ws_stride;
  double *pts = reinterpret_cast<double *>(ws + y.ws_floats);  // (ws_floats and ws_stride are multiples of 4 floats)
  float *fval = ws + y.ws_floats + 2 * LB_WAVES * D;
  const float *dx = ws + y.o_dx;
  Src<double> src;
  src.X = pts;
  src.row_stride = D;
  src.x_step = 0;
  bore::stream_restart_drive(
      a.r, D,
      [&] {
        for (int i = threadIdx.x; i < LB_WAVES * D; i += NTH) pts[i] = 0.0;  // (rows of waves that never ask)
        for (int b = threadIdx.x; b < ROWS; b += NTH) rows[b] = b < NW ? b : 0;
      },
      [&](const int wv, const int lane, const double *x) {
        for (int d = lane; d < D; d += 64) pts[wv * D + d] = x[d];
      },
      [&] {
        tile_value_grad(S, y, th, ws, src, rows, NW, a.T, a.r.transform, a.r.sign,
                        [&](const int b, const float v) { fval[b] = v; });
      },
      [&](const int wv, const int lane, double &f, double *g) {
        f = (double)fval[wv];
        for (int d = lane; d < D; d += 64) g[d] = (double)dx[wv * D + d];
      });
}

struct SFitArgs {
  SLay y;
  float *theta, *am, *av;
  long long *at;
  const float *X, *Y;
  const int *perm;
  float *epoch_loss, *ws;
  long long N;
  int T, epochs, B;
  float mask_value, lr, beta1, beta2, eps;
};

// ONE workgroup per model, every Adam step of the call in one launch.
__global__ void __launch_bounds__(NTH) lstm_stream_fit_kernel(const SFitArgs A) {
  __shared__ StreamLds S;
  __shared__ int rows[ROWS];
  const SLay &y = A.y;
  const Lay &a = y.a;
  const int tid = threadIdx.x, T = A.T, H = a.H, G = a.G, L = a.L;
  const long long m = blockIdx.x, N = A.N;
  float *th = A.theta + m * a.P, *mg = A.am + m * a.P, *vg = A.av + m * a.P;
  float *ws = A.ws + m * y.ws_floats;
  const long long t0 = A.at[m];
  AdamClock clock(A.beta1, A.beta2, t0);
  const float omb1 = 1.f - A.beta1, omb2 = 1.f - A.beta2, eps = A.eps;
  const bool with_l2 = any_l2(a);
  Src<float> src;
  src.X = A.X + m * N * T * a.D;
  src.row_stride = (long long)T * a.D;
  src.x_step = a.D;
  const float *Y = A.Y + m * N * T;
  long long steps = 0;
  for (int e = 0; e < A.epochs; ++e) {
    double eloss = 0.0;
    const int *pe = A.perm + (m * A.epochs + e) * N;
    for (long long s0 = 0; s0 < N; s0 += A.B) {
      const int nr = (int)min((long long)A.B, N - s0);
      __syncthreads();
      for (int b = tid; b < ROWS; b += NTH) rows[b] = b < nr ? pe[s0 + b] : 0;
      __syncthreads();
      tile_begin(y, ws, src, rows, nr, T, 1, A.mask_value);
      tile_forward(S, y, th, ws, src, rows, nr, T);
      const float bce = tile_bce(S, y, ws, Y, rows, nr, T, 1.f / (float)(nr * T));
      const float penalty = with_l2 ? tile_penalty(S, a, th) : 0.f;  // of the weights this step's loss sees
      tile_backward(S, y, th, ws, nr, T, false);
      // Adam (ResourceApplyAdam) in the epilogue of each gradient product; every delta above came from the old theta
      ++steps;
      const float alpha = clock.advance(A.lr, A.beta1, A.beta2);
      auto adam = [&](const int p, const float f, const float grad) {
        float mm = mg[p], vv = vg[p];
        th[p] = adam_update_ieee(th[p], grad, f, mm, vv, alpha, omb1, omb2, eps);
        mg[p] = mm;
        vg[p] = vv;
      };
      for (int l = 0; l < L; ++l) {
        const int in = a.in_dim[l], K1 = in + H + 1, gw = a.gW[l];
        const float l2k = a.l2k[l], l2b = a.l2b[l];
        stream_gemm<true, false>(
            S, K1, G, T * nr, xh_at(y, ws, l, 0, nr), K1, dz_at(y, ws, l, 0, nr), G, [](int, int) { return 0.f; },
            [&](const int i, const int j, const float v) {
              adam(gw + i * G + j, i < in ? l2k : (i < in + H ? 0.f : l2b), v);
            });
      }
      {
        const int gwo = a.gWo;
        const float l2k = a.l2k[L], l2b = a.l2b[L];
        stream_gemm<true, false>(
            S, H + 1, 1, T * nr, ht_at(y, ws, 0, nr), H + 1, ws + y.o_dlogit, 1, [](int, int) { return 0.f; },
            [&](const int i, int, const float v) { adam(gwo + i, i < H ? l2k : l2b, v); });
      }
      eloss += (double)(bce / (float)(nr * T) + penalty) * nr;
    }
    if (A.epoch_loss && tid == 0) A.epoch_loss[m * A.epochs + e] = (float)(eloss / (double)N);
  }
  if (tid == 0) A.at[m] = t0 + steps;
}

struct SEvalArgs {
  SLay y;
  const float *theta, *X, *Y;
  long long N;
  int T;
  float mask_value;
  float *part;  // [models][tiles][3]: the tile's loss sum, hits, live elements
  float *loss, *acc, *ws;
};

__global__ void __launch_bounds__(NTH) lstm_stream_evaluate_kernel(const SEvalArgs A) {
  __shared__ StreamLds S;
  __shared__ int rows[ROWS];
  const SLay &y = A.y;
  const Lay &a = y.a;
  const int tid = threadIdx.x, T = A.T;
  const long long m = blockIdx.x, N = A.N;
  const float *th = A.theta + m * a.P;
  float *ws = A.ws + (m * gridDim.y + blockIdx.y) * y.ws_floats;
  const long long n_tiles = (N + ROWS - 1) / ROWS;
  Src<float> src;
  src.X = A.X + m * N * T * a.D;
  src.row_stride = (long long)T * a.D;
  src.x_step = a.D;
  const float *Y = A.Y + m * N * T;
  for (long long tile = blockIdx.y; tile < n_tiles; tile += gridDim.y) {
    const long long s0 = tile * ROWS;
    const int nr = (int)min((long long)ROWS, N - s0);
    for (int b = tid; b < ROWS; b += NTH) rows[b] = (int)(s0 + (b < nr ? b : 0));
    __syncthreads();
    tile_begin(y, ws, src, rows, nr, T, 1, A.mask_value);
    tile_forward(S, y, th, ws, src, rows, nr, T);
    const float bce = tile_bce(S, y, ws, Y, rows, nr, T, 0.f);
    // binary_accuracy on the model output (the logit) at 0.5, weighted by the mask
    const float *mask = ws + y.o_mask, *logit = ws + y.o_logit;
    float h = 0.f, n = 0.f;
    for (int it = tid; it < nr * T; it += NTH) {
      const int t = it / nr, b = it - t * nr;
      masked_hit(logit[it], Y[(long long)rows[b] * T + t], mask[it] != 0.f, h, n);
    }
    const float hs = stream_wg_sum(S, h), ns = stream_wg_sum(S, n);
    if (tid == 0) {
      float *p = A.part + (m * n_tiles + tile) * 3;
      p[0] = bce; p[1] = hs; p[2] = ns;
    }
    __syncthreads();
  }
}

// The tiles' sums in tile order and the penalty: one workgroup per model, behind the kernel above on the stream.
__global__ void __launch_bounds__(NTH) lstm_stream_evaluate_finish_kernel(const SEvalArgs A) {
  __shared__ StreamLds S;
  const Lay &a = A.y.a;
  const long long m = blockIdx.x, n_tiles = (A.N + ROWS - 1) / ROWS;
  const float penalty = tile_penalty(S, a, A.theta + m * a.P);
  if (threadIdx.x == 0) {
    double tot = 0.0, hit = 0.0, live_n = 0.0;
    const float *p = A.part + m * n_tiles * 3;
    for (long long i = 0; i < n_tiles; ++i) {
      tot += (double)p[3 * i]; hit += (double)p[3 * i + 1]; live_n += (double)p[3 * i + 2];
    }
    A.loss[m] = (float)(tot / ((double)A.N * A.T)) + penalty;
    A.acc[m] = live_n > 0 ? (float)(hit / live_n) : 0.f;
  }
}

}  // namespace bore_lstm_stream

// --------------------------------------------------------------------------------------------------
// C ABI
// --------------------------------------------------------------------------------------------------
namespace bls = bore_lstm_stream;

extern "C" int bore_lstm_streamed(const bore_lstm_desc *desc, int T) {
  if (T < 1) return fail(BORE_E_INVALID, "lstm_streamed: need at least one step (got %d)", T);
  Lay a;
  const int rc = make_lay(desc, T, &a);
  if (rc != BORE_E_UNSUPPORTED) return rc;  // (0: the LDS flavour takes it; else a bad descriptor)
  bls::SLay y;
  if (const int rs = bls::stream_lay(desc, T, bls::WS_FORWARD, &y)) return rs;  // (neither: the bound by name)
  g_bore_err[0] = 0;  // (the LDS refusal is this query's answer, not its error)
  return 1;
}

extern "C" int bore_lstm_stream_forward(const bore_lstm_desc *desc, int n_models, const float *theta, const float *X,
                                        int64_t n_rows, int T, int many_to_many, float mask_value, float *out,
                                        void *stream) {
  bls::SFwdArgs A;
  const int rc = lstm_forward_request(
      "lstm_stream_forward", A, [&] { return bls::stream_lay(desc, T, bls::WS_FORWARD, &A.y); }, n_models, theta, X,
      n_rows, T, many_to_many, mask_value, out);
  if (rc) return rc < 0 ? rc : 0;
  const long long gy = stream_walkers(n_models, (n_rows + bls::ROWS - 1) / bls::ROWS, A.y.ws_floats, true);
  return with_workspace((size_t)n_models * gy * A.y.ws_floats, stream, "lstm_stream_forward_kernel", [&](float *ws) {
    A.ws = ws;
    hipLaunchKernelGGL(bls::lstm_stream_forward_kernel, dim3(n_models, (unsigned)gy), dim3(bls::NTH), 0,
                       (hipStream_t)stream, A);
    return 0;
  });
}

extern "C" int bore_lstm_stream_value_and_input_grad(const bore_lstm_desc *desc, int n_models, const float *theta,
                                                     const double *X, int64_t n_rows, int num_steps, int transform,
                                                     int negate, float *val, double *grad, void *stream) {
  bls::SVgArgs A;
  const int rc = lstm_value_grad_request(
      "lstm_stream_value_and_input_grad", A, [&] { return bls::stream_lay(desc, num_steps, bls::WS_VALUE_GRAD, &A.y); },
      n_models, theta, X, n_rows, num_steps, transform, val, grad);
  if (rc) return rc < 0 ? rc : 0;
  A.sign = negate ? -1.f : 1.f;
  const long long gy = stream_walkers(n_models, (n_rows + bls::ROWS - 1) / bls::ROWS, A.y.ws_floats, true);
  return with_workspace((size_t)n_models * gy * A.y.ws_floats, stream, "lstm_stream_value_grad_kernel", [&](float *ws) {
    A.ws = ws;
    hipLaunchKernelGGL(bls::lstm_stream_value_grad_kernel, dim3(n_models, (unsigned)gy), dim3(bls::NTH), 0,
                       (hipStream_t)stream, A);
    return 0;
  });
}

extern "C" int bore_lstm_stream_fit(const bore_lstm_desc *desc, int n_models, float *theta, float *adam_m,
                                    float *adam_v, int64_t *adam_t, const float *X, const float *y, int64_t N, int T,
                                    float mask_value, int epochs, int batch_size, const int32_t *perm,
                                    const bore_adam_cfg *adam, float *epoch_loss, void *stream) {
  bls::SFitArgs A;
  const int rc = lstm_fit_request(
      "lstm_stream_fit", A, [&] { return bls::stream_lay(desc, T, bls::WS_FIT, &A.y); }, n_models, theta, adam_m, adam_v,
      adam_t, X, y, N, T, mask_value, epochs, batch_size, perm, adam, epoch_loss);
  if (rc) return rc < 0 ? rc : 0;
  return with_workspace((size_t)n_models * A.y.ws_floats, stream, "lstm_stream_fit_kernel", [&](float *ws) {
    A.ws = ws;
    hipLaunchKernelGGL(bls::lstm_stream_fit_kernel, dim3(n_models), dim3(bls::NTH), 0, (hipStream_t)stream, A);
    return 0;
  });
}

extern "C" int bore_lstm_stream_evaluate(const bore_lstm_desc *desc, int n_models, const float *theta, const float *X,
                                         const float *y, int64_t N, int T, float mask_value, float *loss, float *acc,
                                         void *stream) {
  bls::SEvalArgs A;
  if (const int rc = lstm_evaluate_request(
          "lstm_stream_evaluate", A, [&] { return bls::stream_lay(desc, T, bls::WS_FORWARD, &A.y); }, n_models, theta, X,
          y, N, T, mask_value, loss, acc))
    return rc;
  if (N > 0x7fffffffLL) return fail(BORE_E_UNSUPPORTED, "lstm_stream_evaluate: N > 2^31 - 1");
  const long long tiles = (N + bls::ROWS - 1) / bls::ROWS;
  const long long gy = stream_walkers(n_models, tiles, A.y.ws_floats, true);
  const size_t n_ws = (size_t)n_models * gy * A.y.ws_floats, n_part = (size_t)n_models * tiles * 3;
  hipStream_t st = (hipStream_t)stream;
  return with_workspace(n_ws + n_part, stream, "lstm_stream_evaluate_kernel", [&](float *buf) {
    A.ws = buf;
    A.part = buf + n_ws;
    hipLaunchKernelGGL(bls::lstm_stream_evaluate_kernel, dim3(n_models, (unsigned)gy), dim3(bls::NTH), 0, st, A);
    if (hipPeekAtLastError() == hipSuccess)  // (an error stays for the check behind this)
      hipLaunchKernelGGL(bls::lstm_stream_evaluate_finish_kernel, dim3(n_models), dim3(bls::NTH), 0, st, A);
    return 0;
  });
}

// ---- acquisition: screening and restarts ---------------------------------------------------------------------------
// The requests of the two entry points, in the order of lstm_*_request (bore_lstm.hip): n_models and T, the streamed
// bounds (stream_lay into A.y), D <= BORE_DIM_MAX, the candidates and the starts, the options and the box, and only
// then the device pointers.  No HIP call.
template <class LayFn>
static int lstm_acq_common(const char *who, int n_models, int T, LayFn lay, const bls::SLay &y) {
  if (const int rc = lstm_common(who, n_models, T, lay)) return rc;
  if (y.a.D > BORE_DIM_MAX)
    return fail(BORE_E_UNSUPPORTED, "%s: screening and restarts take D <= BORE_DIM_MAX = %d (got %d)", who, BORE_DIM_MAX,
                y.a.D);
  return 0;
}

static int lstm_screen_request(const char *who, bls::SScreenArgs &A, const bore_lstm_desc *desc, int n_models,
                               const float *theta, const double *X_init, int64_t n_samples, int x_shared, int T,
                               int num_starts, const double *x0, const int32_t *idx) {
  if (const int rc = lstm_acq_common(
          who, n_models, T, [&] { return bls::stream_lay(desc, T, bls::WS_FORWARD, &A.y); }, A.y))
    return rc;
  if (n_samples < 1) return fail(BORE_E_INVALID, "%s: n_samples out of range", who);
  if (n_samples > BORE_STREAM_MAX_SAMPLES)
    return fail(BORE_E_UNSUPPORTED,
                "%s: the selection ranks n_samples <= BORE_STREAM_MAX_SAMPLES = %d sort keys in one workgroup's LDS "
                "(got %lld)", who, BORE_STREAM_MAX_SAMPLES, (long long)n_samples);
  if (num_starts < 1 || num_starts > n_samples)
    return fail(BORE_E_INVALID, "%s: need 1 <= num_starts <= n_samples", who);
  if (!theta || !X_init || !x0 || !idx) return fail(BORE_E_INVALID, "%s: null pointer", who);
  A.theta = theta; A.X = X_init; A.n = n_samples; A.T = T; A.x_shared = x_shared ? 1 : 0;
  return 0;
}

static int lstm_lbfgsb_request(const char *who, bls::SLbfgsbArgs &A, const bore_lstm_desc *desc, int n_models,
                               const float *theta, int T, int transform, const double *x0, int num_starts,
                               const double *lb, const double *ub, const bore_lbfgsb_opts *opts, double *x, double *fun,
                               double *jac, int32_t *info) {
  if (const int rc = lstm_acq_common(
          who, n_models, T, [&] { return bls::stream_lay(desc, T, bls::WS_VALUE_GRAD, &A.y); }, A.y))
    return rc;
  if (num_starts < 1) return fail(BORE_E_INVALID, "%s: num_starts < 1", who);
  if (!lb || !ub || !opts) return fail(BORE_E_INVALID, "%s: null pointer (bounds, options)", who);
  if (const int rc = lbfgsb_convert(A.y.a.D, transform, num_starts, lb, ub, opts, A.r.box, A.r.nbd, A.r.opt)) return rc;
  if (!theta || !x0 || !x || !fun || !jac || !info) return fail(BORE_E_INVALID, "%s: null pointer", who);
  A.theta = theta; A.r.x0 = x0; A.r.x = x; A.r.fun = fun; A.r.jac = jac; A.r.info = info;
  A.r.R = num_starts; A.T = T; A.r.transform = transform;
  return 0;
}

extern "C" int bore_lstm_stream_screen_topk(const bore_lstm_desc *desc, int n_models, const float *theta,
                                            const double *X_init, int64_t n_samples, int x_shared, int T,
                                            int num_starts, double *x0, int32_t *idx, float *pred, void *stream) {
  static const char who[] = "lstm_stream_screen_topk";
  bls::SScreenArgs A;
  if (const int rc = lstm_screen_request(who, A, desc, n_models, theta, X_init, n_samples, x_shared, T, num_starts, x0,
                                         idx))
    return rc;
  // the predictions: bore_lstm_stream_forward's geometry and workspace rule; the selection: the Dense flavour's stage
  StreamSampleArgs sp;
  sp.sampled = 0; sp.seed = 0; sp.model0 = 0; sp.draw = 0;
  return stream_screen_tail(who, n_models, n_samples, num_starts, A.y.a.D, A.x_shared, X_init, sp, A.y.ws_floats, x0,
                            idx, pred, stream, [&](float *ws, float *out, long long gy) {
                              A.ws = ws;
                              A.out = out;
                              hipLaunchKernelGGL(bls::lstm_stream_screen_pred_kernel, dim3(n_models, (unsigned)gy),
                                                 dim3(bls::NTH), 0, (hipStream_t)stream, A);
                            });
}

extern "C" int bore_lstm_stream_lbfgsb_minimize(const bore_lstm_desc *desc, int n_models, const float *theta, int T,
                                                int transform, int negate, const double *x0, int num_starts,
                                                const double *lb, const double *ub, const bore_lbfgsb_opts *opts,
                                                double *x, double *fun, double *jac, int32_t *info, void *stream) {
  static const char who[] = "lstm_stream_lbfgsb_minimize";
  bls::SLbfgsbArgs A;
  if (const int rc = lstm_lbfgsb_request(who, A, desc, n_models, theta, T, transform, x0, num_starts, lb, ub, opts, x,
                                         fun, jac, info))
    return rc;
  A.r.sign = negate ? -1.f : 1.f;
  // static LDS: the panels and the rows.  Per workgroup: the value + gradient tile, then the four fp64 points and
  // their four values.
  const int D = A.y.a.D;
  static_assert(bls::LB_WAVES == BORE_THREADS / 64, "stream_restart_launch's wave limit");
  return stream_restart_launch(who, "lstm_stream_lbfgsb_kernel", bls::lstm_stream_lbfgsb_kernel, A, D,
                               sizeof(StreamLds) + bls::ROWS * sizeof(int), n_models,
                               A.y.ws_floats + 2 * bls::LB_WAVES * D + bls::LB_WAVES, opts, stream);
}
