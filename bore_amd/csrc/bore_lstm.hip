// bore_lstm.hip -- the multi-fidelity classifier of the reference (bore/models.py:48-104,
// StackedRecurrentFactory): a stack of Keras LSTMCells and a Dense(1) head, run over the rungs of a
// Hyperband ladder.  Entry points: bore_lstm_param_count / _forward / _value_and_input_grad / _fit /
// _evaluate (include/bore_hip.h).  Included from bore_all.hip.
//
// One scheme for every entry point: a workgroup of LSTM_NT threads takes a TILE of up to 64 sequences
// and walks them through time, layer after layer, with the packed parameters in LDS (rows of W and U
// padded to 4H + 1 floats, so the transposed products of the backward pass are free of bank
// conflicts).  Work inside a (step, layer) phase is split over (sequence, unit) items: one thread
// forms the four gate sums of its unit, in a fixed order, so that every form of the forward pass --
// many-to-many, one-to-one, inside the fit -- gives the same bits for the same inputs.  A masked step
// keeps h and c (Keras RNN with a Masking layer, TF 2.5): chosen by select, never by a branch per row.
// The backward pass (fit, input gradient) reads the activations of the whole sequence back from a
// per-tile device workspace (stream-ordered, hipMallocAsync), accumulates the weight gradients of an
// Adam step in a per-model device buffer in a fixed order, and updates theta (LDS), m and v (memory)
// once per step -- every Adam step of a call inside one launch, as the Dense fit does.
// This is the LDS flavour: what does not fit one CU's LDS is refused here and taken by the streamed flavour,
// bore_lstm_stream.hip (entry points of its own).  The two share the scalar arithmetic of a cell and of the loss
// (lstm_math.h; the Adam update: mlp_math.h's adam_update_ieee), the packed layout and the request checks below.
#include "host_common.h"
#include "lstm_math.h"

namespace bore_lstm {

using bore::AdamClock, bore::adam_update_ieee, bore::objective_transform;

constexpr int NT = 512;           // threads per workgroup (8 waves)
constexpr int TILE = 64;          // sequences per tile (batch_size <= 64)
constexpr int MAXL = BORE_LSTM_MAX_LAYERS;
constexpr int MAXH = BORE_LSTM_MAX_UNITS;
constexpr int MAXT = BORE_LSTM_MAX_STEPS;
constexpr int MAXD = BORE_LSTM_MAX_INPUT;
constexpr int MAXITEMS = TILE * MAXH / NT;  // (sequence, unit) items per thread

struct Lay {
  int D, L, H, act, T, G, G1;  // G = 4H, G1 = padded row of W / U in LDS
  int P;
  int in_dim[MAXL];
  int gW[MAXL], gU[MAXL], gb[MAXL], gWo, gbo;  // offsets in the packed vector (get_weights order)
  int sW[MAXL], sU[MAXL], sb[MAXL], sWo, sbo;  // offsets in LDS
  int o_h, o_c, o_dz, o_din, o_dx, o_logit, o_dlogit, o_mask, o_red, o_rows, lds_floats;
  float l2k[MAXL + 1], l2b[MAXL + 1];  // index L: the Dense head
  long long ws_floats;                 // activations of one tile: gates [L][T][64][4H], c, h [L][T][64][H]
};

// --------------------------------------------------------------------------------------------------
// host: descriptor -> layout
// --------------------------------------------------------------------------------------------------
// What either flavour does with a descriptor: a descriptor of the BORE classifier, within the flavour's bounds (`who`:
// "lstm" / "lstm_stream"; its two maxima and the names of their macros), then the network and where its pieces start
// in the packed vector.
static int lay_packed(const bore_lstm_desc *d, int T, const char *who, int max_in, const char *max_in_name, int max_h,
                      const char *max_h_name, Lay &a) {
  if (!d) return fail(BORE_E_INVALID, "lstm: null descriptor");
  if (d->output_dim != 1)
    return fail(BORE_E_UNSUPPORTED, "lstm: output_dim must be 1 (the BORE classifier), got %d", d->output_dim);
  if (d->input_dim < 1 || d->n_layers < 1 || d->units < 1)
    return fail(BORE_E_INVALID, "lstm: input_dim, n_layers and units must be positive (got %d, %d, %d)",
                d->input_dim, d->n_layers, d->units);
  if (d->act < BORE_ACT_LINEAR || d->act > BORE_ACT_TANH)
    return fail(BORE_E_INVALID, "lstm: unknown activation %d", d->act);
  if (d->input_dim > max_in)
    return fail(BORE_E_UNSUPPORTED, "%s: input_dim %d > %d (%s)", who, d->input_dim, max_in, max_in_name);
  if (d->n_layers > MAXL)
    return fail(BORE_E_UNSUPPORTED, "%s: n_layers %d > %d (BORE_LSTM_MAX_LAYERS)", who, d->n_layers, MAXL);
  if (d->units > max_h) return fail(BORE_E_UNSUPPORTED, "%s: units %d > %d (%s)", who, d->units, max_h, max_h_name);
  if (T < 0 || T > MAXT) return fail(BORE_E_UNSUPPORTED, "%s: %d steps > %d (BORE_LSTM_MAX_STEPS)", who, T, MAXT);
  a.D = d->input_dim; a.L = d->n_layers; a.H = d->units; a.act = d->act; a.T = T < 1 ? 1 : T;
  a.G = 4 * a.H; a.G1 = a.G + 1;
  long long g = 0;
  for (int l = 0; l < a.L; ++l) {
    const int in = l == 0 ? a.D : a.H;
    a.in_dim[l] = in;
    a.gW[l] = (int)g; g += (long long)in * a.G;
    a.gU[l] = (int)g; g += (long long)a.H * a.G;
    a.gb[l] = (int)g; g += a.G;
    a.l2k[l] = d->l2_kernel[l]; a.l2b[l] = d->l2_bias[l];
  }
  a.gWo = (int)g; g += a.H; a.gbo = (int)g; g += 1;
  a.l2k[a.L] = d->l2_kernel[a.L]; a.l2b[a.L] = d->l2_bias[a.L];
  a.P = (int)g;
  return 0;
}

static int make_lay(const bore_lstm_desc *d, int T, Lay *y) {
  Lay &a = *y;
  if (const int rc = lay_packed(d, T, "lstm", MAXD, "BORE_LSTM_MAX_INPUT", MAXH, "BORE_LSTM_MAX_UNITS", a)) return rc;
  long long s = 0;
  for (int l = 0; l < a.L; ++l) {
    a.sW[l] = (int)s; s += (long long)a.in_dim[l] * a.G1;
    a.sU[l] = (int)s; s += (long long)a.H * a.G1;
    a.sb[l] = (int)s; s += a.G;
  }
  a.sWo = (int)s; s += a.H; a.sbo = (int)s; s += 1;
  s = (s + 3) & ~3LL;
  const int Dm = a.D > a.H ? a.D : a.H;
  a.o_h = (int)s; s += (long long)a.L * TILE * a.H;
  a.o_c = (int)s; s += (long long)a.L * TILE * a.H;
  a.o_dz = (int)s; s += (long long)TILE * a.G;
  a.o_din = (int)s; s += (long long)TILE * Dm;
  a.o_dx = (int)s; s += (long long)TILE * a.D;
  a.o_logit = (int)s; s += (long long)TILE * a.T;
  a.o_dlogit = (int)s; s += (long long)TILE * a.T;
  a.o_mask = (int)s; s += (long long)TILE * a.T;
  a.o_red = (int)s; s += NT;
  a.o_rows = (int)s; s += TILE;
  a.lds_floats = (int)s;
  if (s * 4 > BORE_LDS_BYTES)
    return fail(BORE_E_UNSUPPORTED,
                "lstm: %d inputs, %d layers of %d units over %d steps need %lld B of LDS per workgroup "
                "(> %d): parameters (%d floats) and one tile of state must fit one CU",
                a.D, a.L, a.H, a.T, s * 4, BORE_LDS_BYTES, a.P);
  a.ws_floats = (long long)a.L * a.T * TILE * (a.G + 2 * a.H);
  return 0;
}

// --------------------------------------------------------------------------------------------------
// device
// --------------------------------------------------------------------------------------------------
// LDS address of packed parameter p
__device__ __forceinline__ int lds_of(const Lay &a, int p) {
  for (int l = 0; l < a.L; ++l) {
    if (p < a.gU[l] && p >= a.gW[l]) { const int q = p - a.gW[l]; return a.sW[l] + (q / a.G) * a.G1 + q % a.G; }
    if (p < a.gb[l] && p >= a.gU[l]) { const int q = p - a.gU[l]; return a.sU[l] + (q / a.G) * a.G1 + q % a.G; }
    if (p < a.gb[l] + a.G && p >= a.gb[l]) return a.sb[l] + (p - a.gb[l]);
  }
  return a.sWo + (p - a.gWo);  // (Wo and bo are adjacent in both)
}

// l2 factor of packed parameter p (never U: Keras' recurrent_regularizer is not set)
__device__ __forceinline__ float l2_of(const Lay &a, int p) {
  for (int l = 0; l < a.L; ++l) {
    if (p < a.gU[l] && p >= a.gW[l]) return a.l2k[l];
    if (p < a.gb[l] && p >= a.gU[l]) return 0.f;
    if (p < a.gb[l] + a.G && p >= a.gb[l]) return a.l2b[l];
  }
  return p == a.gbo ? a.l2b[a.L] : a.l2k[a.L];
}

__device__ __forceinline__ void load_theta(const Lay &a, const float *__restrict__ g, float *sm) {
  for (int p = threadIdx.x; p < a.P; p += NT) sm[lds_of(a, p)] = g[p];
}

// fixed-order sum over the workgroup (tree over the LSTM_NT slots); every thread gets the result
__device__ __forceinline__ float block_sum(float v, float *red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  const float r = red[0];
  __syncthreads();
  return r;
}

// Where a tile's inputs come from.  X points at [rows][T][D] (x_step = D) or at [rows][D] repeated
// over the steps (x_step = 0, RepeatVector of the one-to-one net); rows[b] is the row of sequence b.
template <typename XT>
struct Src {
  const XT *X;
  long long row_stride;
  int x_step;
  __device__ __forceinline__ float x(const int *rows, int b, int t, int k) const {
    return (float)X[(long long)rows[b] * row_stride + (long long)t * x_step + k];
  }
};

// mask[b][t] = 1 iff any feature of step t differs from mask_value (Keras Masking); use_mask = 0: all live
template <typename XT>
__device__ __forceinline__ bool step_live(const Lay &a, const Src<XT> &src, const int *rows, int b, int t, int use_mask,
                                          float mask_value) {
  bool live = !use_mask;
  if (use_mask)
    for (int k = 0; k < a.D; ++k) live |= src.x(rows, b, t, k) != mask_value;
  return live;
}

template <typename XT>
__device__ void make_mask(const Lay &a, const Src<XT> &src, const int *rows, int nrows, int T, int use_mask,
                          float mask_value, float *mask) {
  for (int it = threadIdx.x; it < nrows * T; it += NT) {
    const int b = it / T, t = it % T;
    mask[b * T + t] = step_live(a, src, rows, b, t, use_mask, mask_value) ? 1.f : 0.f;
  }
}

// Forward pass of one tile over T steps: logits [b][t] in LDS; with ws, the activations for backward.
template <typename XT>
__device__ void tile_forward(const Lay &a, float *sm, const Src<XT> &src, int nrows, int T, float *ws) {
  const int H = a.H, G = a.G, G1 = a.G1, L = a.L;
  const int *rows = reinterpret_cast<const int *>(sm + a.o_rows);
  const float *mask = sm + a.o_mask;
  float *hS = sm + a.o_h, *cS = sm + a.o_c, *logit = sm + a.o_logit;
  for (int i = threadIdx.x; i < L * TILE * H; i += NT) hS[i] = cS[i] = 0.f;
  __syncthreads();
  const int n_items = nrows * H;
  for (int t = 0; t < T; ++t) {
    for (int l = 0; l < L; ++l) {
      const int in_dim = a.in_dim[l];
      const float *W = sm + a.sW[l], *U = sm + a.sU[l], *bias = sm + a.sb[l];
      float *hl = hS + l * TILE * H, *cl = cS + l * TILE * H;
      const float *hin = l > 0 ? hS + (l - 1) * TILE * H : hS;  // (l > 0: layer l-1 at this step)
      float hn[MAXITEMS], cn[MAXITEMS];
#pragma unroll
      for (int q = 0; q < MAXITEMS; ++q) {
        const int it = threadIdx.x + q * NT;
        if (it >= n_items) break;
        const int b = it / H, u = it % H;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;  // x . W
        for (int k = 0; k < in_dim; ++k) {
          const float xv = l == 0 ? src.x(rows, b, t, k) : hin[b * H + k];
          const float *w = W + k * G1 + u;
          s0 = fmaf(xv, w[0], s0); s1 = fmaf(xv, w[H], s1); s2 = fmaf(xv, w[2 * H], s2); s3 = fmaf(xv, w[3 * H], s3);
        }
        float r0 = 0.f, r1 = 0.f, r2 = 0.f, r3 = 0.f;  // h . U
        for (int k = 0; k < H; ++k) {
          const float hv = hl[b * H + k];
          const float *w = U + k * G1 + u;
          r0 = fmaf(hv, w[0], r0); r1 = fmaf(hv, w[H], r1); r2 = fmaf(hv, w[2 * H], r2); r3 = fmaf(hv, w[3 * H], r3);
        }
        const Gates g = gates_of(a.act, (s0 + r0) + bias[u], (s1 + r1) + bias[H + u], (s2 + r2) + bias[2 * H + u],
                                 (s3 + r3) + bias[3 * H + u]);
        const float cp = cl[b * H + u];
        // two products and a sum, three roundings; the streamed flavour forms fmaf(f, cp, i * g), two
        const float c = g.f * cp + g.i * g.g;
        cell_out(a.act, g.o, c, cp, hl[b * H + u], mask[b * T + t] != 0.f, cn[q], hn[q]);
        if (ws) {
          float *gw = ws + (((long long)l * a.T + t) * TILE + b) * G;
          gw[u] = g.i; gw[H + u] = g.f; gw[2 * H + u] = g.g; gw[3 * H + u] = g.o;
        }
      }
      __syncthreads();
#pragma unroll
      for (int q = 0; q < MAXITEMS; ++q) {
        const int it = threadIdx.x + q * NT;
        if (it >= n_items) break;
        hl[it] = hn[q];
        cl[it] = cn[q];
        if (ws) {
          const long long base = (long long)L * a.T * TILE * G;
          const long long o = ((long long)l * a.T + t) * TILE * H + it;
          ws[base + o] = cn[q];                               // c history
          ws[base + (long long)L * a.T * TILE * H + o] = hn[q];  // h history
        }
      }
      __syncthreads();
    }
    // Dense head on the top layer's output
    const float *Wo = sm + a.sWo, bo = sm[a.sbo];
    const float *ht = hS + (L - 1) * TILE * H;
    for (int b = threadIdx.x; b < nrows; b += NT) {
      float s = 0.f;
      for (int k = 0; k < H; ++k) s = fmaf(ht[b * H + k], Wo[k], s);
      logit[b * T + t] = s + bo;
    }
  }
  __syncthreads();
}

__device__ __forceinline__ const float *ws_c(const Lay &a, const float *ws, int l, int t) {
  return ws + (long long)a.L * a.T * TILE * a.G + ((long long)l * a.T + t) * TILE * a.H;
}
__device__ __forceinline__ const float *ws_h(const Lay &a, const float *ws, int l, int t) {
  return ws + (long long)a.L * a.T * TILE * (a.G + a.H) + ((long long)l * a.T + t) * TILE * a.H;
}

// Backpropagation through time of one tile, from dlogit [b][t] (LDS).  gacc != null: adds the weight
// gradients to gacc (packed order); want_dx: dx [b][k] (LDS) = d/dx summed over the steps.
template <typename XT>
__device__ void tile_backward(const Lay &a, float *sm, const Src<XT> &src, int nrows, int T, const float *ws,
                              float *gacc, bool want_dx) {
  const int H = a.H, G = a.G, G1 = a.G1, L = a.L;
  const int *rows = reinterpret_cast<const int *>(sm + a.o_rows);
  const float *mask = sm + a.o_mask, *dlogit = sm + a.o_dlogit;
  float *dhS = sm + a.o_h, *dcS = sm + a.o_c, *dz = sm + a.o_dz, *din = sm + a.o_din, *dx = sm + a.o_dx;
  const float *Wo = sm + a.sWo;
  for (int i = threadIdx.x; i < L * TILE * H; i += NT) dhS[i] = dcS[i] = 0.f;
  if (want_dx)
    for (int i = threadIdx.x; i < TILE * a.D; i += NT) dx[i] = 0.f;
  // the head: dWo[k] = sum_t sum_b dlogit h_top, dbo = sum dlogit
  if (gacc) {
    for (int k = threadIdx.x; k <= H; k += NT) {
      float s = 0.f;
      for (int t = T - 1; t >= 0; --t) {
        const float *ht = ws_h(a, ws, L - 1, t);
        for (int b = 0; b < nrows; ++b) s = fmaf(dlogit[b * T + t], k < H ? ht[b * H + k] : 1.f, s);
      }
      gacc[a.gWo + k] += s;
    }
  }
  __syncthreads();
  const int n_items = nrows * H;
  for (int t = T - 1; t >= 0; --t) {
    for (int l = L - 1; l >= 0; --l) {
      const int in_dim = a.in_dim[l];
      float *dhl = dhS + l * TILE * H, *dcl = dcS + l * TILE * H;
      const float *gts = ws + ((long long)l * a.T + t) * TILE * G;
      const float *ct = ws_c(a, ws, l, t);
      const float *cpv = t > 0 ? ws_c(a, ws, l, t - 1) : nullptr;
      // phase A: the gate deltas of (sequence, unit) items
      for (int it = threadIdx.x; it < n_items; it += NT) {
        const int b = it / H, u = it % H;
        const float above = l == L - 1 ? dlogit[b * T + t] * Wo[u] : din[b * H + u];
        const float dh = dhl[it] + above;
        const bool live = mask[b * T + t] != 0.f;
        const float *g = gts + b * G;
        const GateDeltas dl = gate_deltas(a.act, Gates{g[u], g[H + u], g[2 * H + u], g[3 * H + u]}, ct[it],
                                          cpv ? cpv[it] : 0.f, dh, dcl[it], live);
        float *d = dz + b * G;
        d[u] = dl.zi; d[H + u] = dl.zf; d[2 * H + u] = dl.zg; d[3 * H + u] = dl.zo;
        dcl[it] = dl.c;
        if (!live) dhl[it] = dh;  // (a masked step passes h's gradient to the step before)
      }
      __syncthreads();
      // phase B: recurrent delta, delta of the layer below, weight gradients
      const float *W = sm + a.sW[l], *U = sm + a.sU[l];
      for (int it = threadIdx.x; it < n_items; it += NT) {
        const int b = it / H, k = it % H;
        if (mask[b * T + t] == 0.f) continue;
        const float *d = dz + b * G, *w = U + k * G1;
        float s = 0.f;
        for (int j = 0; j < G; ++j) s = fmaf(d[j], w[j], s);
        dhl[it] = s;
      }
      if (l > 0 || want_dx) {
        for (int it = threadIdx.x; it < nrows * in_dim; it += NT) {
          const int b = it / in_dim, k = it % in_dim;
          const float *d = dz + b * G, *w = W + k * G1;
          float s = 0.f;
          for (int j = 0; j < G; ++j) s = fmaf(d[j], w[j], s);
          if (l > 0) din[b * H + k] = s;
          else dx[b * a.D + k] += s;
        }
      }
      if (gacc) {
        const float *hin = l > 0 ? ws_h(a, ws, l - 1, t) : nullptr;
        const float *hpv = t > 0 ? ws_h(a, ws, l, t - 1) : nullptr;
        const int n_w = (in_dim + H + 1) * G;  // rows of W, rows of U, the bias
        for (int it = threadIdx.x; it < n_w; it += NT) {
          const int r = it / G, j = it % G;
          float s = 0.f;
          if (r < in_dim) {
            for (int b = 0; b < nrows; ++b)
              s = fmaf(l > 0 ? hin[b * H + r] : src.x(rows, b, t, r), dz[b * G + j], s);
            gacc[a.gW[l] + r * G + j] += s;
          } else if (r < in_dim + H) {
            if (hpv) {
              for (int b = 0; b < nrows; ++b) s = fmaf(hpv[b * H + (r - in_dim)], dz[b * G + j], s);
              gacc[a.gU[l] + (r - in_dim) * G + j] += s;
            }
          } else {
            for (int b = 0; b < nrows; ++b) s += dz[b * G + j];
            gacc[a.gb[l] + j] += s;
          }
        }
      }
      __syncthreads();
    }
  }
}

// BCE from logits of one tile (per element max(a,0) - a y + log1p(exp(-|a|)), weighted by the mask),
// dlogit = mask (sigmoid(a) - y) / (nrows T); returns the weighted sum of the element losses.
__device__ float tile_bce(const Lay &a, float *sm, const float *Y, long long y_stride, int nrows, int T,
                          float scale) {
  const int *rows = reinterpret_cast<const int *>(sm + a.o_rows);
  const float *mask = sm + a.o_mask, *logit = sm + a.o_logit;
  float *dlogit = sm + a.o_dlogit;
  float part = 0.f;
  for (int it = threadIdx.x; it < nrows * T; it += NT) {
    const int b = it / T, t = it % T;
    const float x = logit[it], y = Y[(long long)rows[b] * y_stride + t];
    part += masked_bce(x, y, mask[it] != 0.f, scale, dlogit[it]);
  }
  return block_sum(part, sm + a.o_red);
}

// --------------------------------------------------------------------------------------------------
// kernels
// --------------------------------------------------------------------------------------------------
struct FwdArgs {
  Lay a;
  const float *theta, *X;
  long long n;
  int T, m2m, use_mask;
  float mask_value;
  float *out;
};

__global__ void __launch_bounds__(NT) lstm_forward_kernel(FwdArgs A) {
  extern __shared__ float sm[];
  const Lay &a = A.a;
  const int m = blockIdx.y;
  const long long r0 = (long long)blockIdx.x * TILE;
  const int nrows = (int)min((long long)TILE, A.n - r0);
  const int T = A.T;
  load_theta(a, A.theta + (long long)m * a.P, sm);
  int *rows = reinterpret_cast<int *>(sm + a.o_rows);
  for (int b = threadIdx.x; b < TILE; b += NT) rows[b] = (int)(b < nrows ? b : 0);
  Src<float> src;
  src.X = A.X + ((long long)m * A.n + r0) * (A.m2m ? (long long)T * a.D : a.D);
  src.row_stride = A.m2m ? (long long)T * a.D : a.D;
  src.x_step = A.m2m ? a.D : 0;
  __syncthreads();
  make_mask(a, src, rows, nrows, T, A.use_mask, A.mask_value, sm + a.o_mask);
  __syncthreads();
  tile_forward(a, sm, src, nrows, T, nullptr);
  const float *logit = sm + a.o_logit;
  if (A.m2m) {
    float *o = A.out + ((long long)m * A.n + r0) * T;
    for (int i = threadIdx.x; i < nrows * T; i += NT) o[i] = logit[i];
  } else {
    float *o = A.out + (long long)m * A.n + r0;
    for (int b = threadIdx.x; b < nrows; b += NT) o[b] = logit[b * T + T - 1];
  }
}

struct VgArgs {
  Lay a;
  const float *theta;
  const double *X;
  long long n;
  int T, transform, negate;
  float *val, *ws;
  double *grad;
};

__global__ void __launch_bounds__(NT) lstm_value_grad_kernel(VgArgs A) {
  extern __shared__ float sm[];
  const Lay &a = A.a;
  const int m = blockIdx.y;
  const long long r0 = (long long)blockIdx.x * TILE;
  const int nrows = (int)min((long long)TILE, A.n - r0);
  const int T = A.T;
  float *ws = A.ws + ((long long)m * gridDim.x + blockIdx.x) * a.ws_floats;
  load_theta(a, A.theta + (long long)m * a.P, sm);
  int *rows = reinterpret_cast<int *>(sm + a.o_rows);
  for (int b = threadIdx.x; b < TILE; b += NT) rows[b] = (int)(b < nrows ? b : 0);
  Src<double> src;
  src.X = A.X + ((long long)m * A.n + r0) * a.D;
  src.row_stride = a.D;
  src.x_step = 0;
  __syncthreads();
  make_mask(a, src, rows, nrows, T, 0, 0.f, sm + a.o_mask);
  __syncthreads();
  tile_forward(a, sm, src, nrows, T, ws);
  // value and d value / d f at the last step
  const float *logit = sm + a.o_logit;
  float *dlogit = sm + a.o_dlogit;
  for (int i = threadIdx.x; i < nrows * T; i += NT) {
    const int b = i / T, t = i % T;
    if (t != T - 1) { dlogit[i] = 0.f; continue; }
    const float s = A.negate ? -1.f : 1.f;
    float v, dT;
    objective_transform(A.transform, s * logit[i], v, dT);
    A.val[(long long)m * A.n + r0 + b] = v;
    dlogit[i] = s * dT;
  }
  __syncthreads();
  tile_backward(a, sm, src, nrows, T, ws, nullptr, true);
  const float *dx = sm + a.o_dx;
  double *g = A.grad + ((long long)m * A.n + r0) * a.D;
  for (int i = threadIdx.x; i < nrows * a.D; i += NT) g[i] = (double)dx[i];
}

struct FitArgsL {
  Lay a;
  float *theta, *am, *av;
  long long *at;
  const float *X, *Y;
  const int *perm;
  float *epoch_loss, *ws, *gacc;
  long long N;
  int T, epochs, B;
  float mask_value, lr, beta1, beta2, eps;
};

__global__ void __launch_bounds__(NT) lstm_fit_kernel(FitArgsL A) {
  extern __shared__ float sm[];
  const Lay &a = A.a;
  const int m = blockIdx.x, T = A.T;
  const long long N = A.N;
  float *th_g = A.theta + (long long)m * a.P, *m_g = A.am + (long long)m * a.P, *v_g = A.av + (long long)m * a.P;
  float *ws = A.ws + (long long)m * a.ws_floats, *gacc = A.gacc + (long long)m * a.P;
  load_theta(a, th_g, sm);
  const long long t0 = A.at[m];
  AdamClock clock(A.beta1, A.beta2, t0);
  const float omb1 = 1.f - A.beta1, omb2 = 1.f - A.beta2;
  Src<float> src;
  src.X = A.X + (long long)m * N * T * a.D;
  src.row_stride = (long long)T * a.D;
  src.x_step = a.D;
  const float *Y = A.Y + (long long)m * N * T;
  int *rows = reinterpret_cast<int *>(sm + a.o_rows);
  long long steps = 0;
  for (int e = 0; e < A.epochs; ++e) {
    double eloss = 0.0;
    const int *pe = A.perm + ((long long)m * A.epochs + e) * N;
    for (long long s0 = 0; s0 < N; s0 += A.B) {
      const int nrows = (int)min((long long)A.B, N - s0);
      __syncthreads();
      for (int b = threadIdx.x; b < TILE; b += NT) rows[b] = b < nrows ? pe[s0 + b] : 0;
      __syncthreads();
      make_mask(a, src, rows, nrows, T, 1, A.mask_value, sm + a.o_mask);
      __syncthreads();
      tile_forward(a, sm, src, nrows, T, ws);
      const float bce = tile_bce(a, sm, Y, T, nrows, T, 1.f / (float)(nrows * T));
      tile_backward(a, sm, src, nrows, T, ws, gacc, false);
      // Adam (ResourceApplyAdam), the l2 penalties of the loss on the weights before the update
      ++steps;
      const float alpha = clock.advance(A.lr, A.beta1, A.beta2);
      float pen = 0.f;
      for (int p = threadIdx.x; p < a.P; p += NT) {
        const int li = lds_of(a, p);
        const float w = sm[li], f = l2_of(a, p);
        pen = l2_term(f, w, pen);
        float mm = m_g[p], vv = v_g[p];
        sm[li] = adam_update_ieee(w, gacc[p], f, mm, vv, alpha, omb1, omb2, A.eps);
        m_g[p] = mm;
        v_g[p] = vv;
        gacc[p] = 0.f;
      }
      const float penalty = block_sum(pen, sm + a.o_red);
      eloss += (double)(bce / (float)(nrows * T) + penalty) * nrows;
    }
    if (A.epoch_loss && threadIdx.x == 0) A.epoch_loss[(long long)m * A.epochs + e] = (float)(eloss / (double)N);
  }
  __syncthreads();
  for (int p = threadIdx.x; p < a.P; p += NT) th_g[p] = sm[lds_of(a, p)];
  if (threadIdx.x == 0) A.at[m] = t0 + steps;
}

struct EvalArgsL {
  Lay a;
  const float *theta, *X, *Y;
  long long N;
  int T;
  float mask_value;
  float *loss, *acc;
};

__global__ void __launch_bounds__(NT) lstm_evaluate_kernel(EvalArgsL A) {
  extern __shared__ float sm[];
  const Lay &a = A.a;
  const int m = blockIdx.x, T = A.T;
  const long long N = A.N;
  load_theta(a, A.theta + (long long)m * a.P, sm);
  Src<float> src;
  src.X = A.X + (long long)m * N * T * a.D;
  src.row_stride = (long long)T * a.D;
  src.x_step = a.D;
  const float *Y = A.Y + (long long)m * N * T;
  int *rows = reinterpret_cast<int *>(sm + a.o_rows);
  double tot = 0.0, hit = 0.0, live_n = 0.0;
  for (long long s0 = 0; s0 < N; s0 += TILE) {
    const int nrows = (int)min((long long)TILE, N - s0);
    __syncthreads();
    for (int b = threadIdx.x; b < TILE; b += NT) rows[b] = (int)(s0 + (b < nrows ? b : 0));
    __syncthreads();
    make_mask(a, src, rows, nrows, T, 1, A.mask_value, sm + a.o_mask);
    __syncthreads();
    tile_forward(a, sm, src, nrows, T, nullptr);
    const float bce = tile_bce(a, sm, Y, T, nrows, T, 0.f);
    // binary_accuracy on the model output (the logit) at 0.5, weighted by the mask
    const float *mask = sm + a.o_mask, *logit = sm + a.o_logit;
    float h = 0.f, n = 0.f;
    for (int it = threadIdx.x; it < nrows * T; it += NT) {
      const int b = it / T, t = it % T;
      masked_hit(logit[it], Y[(long long)rows[b] * T + t], mask[it] != 0.f, h, n);
    }
    const float hs = block_sum(h, sm + a.o_red), ns = block_sum(n, sm + a.o_red);
    tot += (double)bce;
    hit += (double)hs;
    live_n += (double)ns;
  }
  float pen = 0.f;
  for (int p = threadIdx.x; p < a.P; p += NT) pen = l2_term(l2_of(a, p), sm[lds_of(a, p)], pen);
  const float penalty = block_sum(pen, sm + a.o_red);
  if (threadIdx.x == 0) {
    A.loss[m] = (float)(tot / ((double)N * T)) + penalty;
    A.acc[m] = live_n > 0 ? (float)(hit / live_n) : 0.f;
  }
}

}  // namespace bore_lstm

// --------------------------------------------------------------------------------------------------
// C ABI
// --------------------------------------------------------------------------------------------------
using namespace bore_lstm;

extern "C" int64_t bore_lstm_param_count(const bore_lstm_desc *desc) {
  // (a property of the network: counted for any valid descriptor, also one the kernels do not take)
  if (!desc) return fail(BORE_E_INVALID, "lstm: null descriptor");
  if (desc->input_dim < 1 || desc->n_layers < 1 || desc->units < 1 || desc->output_dim < 1)
    return fail(BORE_E_INVALID, "lstm: input_dim, n_layers, units and output_dim must be positive (got %d, %d, %d, %d)",
                desc->input_dim, desc->n_layers, desc->units, desc->output_dim);
  int64_t P = 0;
  for (int l = 0; l < desc->n_layers; ++l)
    P += (int64_t)((l ? desc->units : desc->input_dim) + desc->units + 1) * 4 * desc->units;
  return P + (int64_t)(desc->units + 1) * desc->output_dim;
}

// The requests of the four entry-point pairs, whichever flavour runs them (`who` names the entry point, A is the
// flavour's kernel-argument struct, the other arguments go by their names in include/bore_hip.h).  Refused in this
// order: n_models, T, the flavour's layout and bounds (`lay`: make_lay / stream_lay into A), pointers, the rest; then
// A is filled.  Returns 1 when there is nothing to do, else 0 or the error.  No HIP call.
template <class LayFn>
static int lstm_common(const char *who, int n_models, int T, LayFn lay) {
  if (n_models < 1) return fail(BORE_E_INVALID, "%s: n_models must be >= 1 (got %d)", who, n_models);
  if (T < 1) return fail(BORE_E_INVALID, "%s: need at least one step (got %d)", who, T);
  return lay();
}

template <class A, class LayFn>
static int lstm_forward_request(const char *who, A &a, LayFn lay, int n_models, const float *theta, const float *X,
                                int64_t n_rows, int T, int many_to_many, float mask_value, float *out) {
  if (const int rc = lstm_common(who, n_models, T, lay)) return rc;
  if (!theta || !X || !out) return fail(BORE_E_INVALID, "%s: null pointer", who);
  if (n_rows < 0) return fail(BORE_E_INVALID, "%s: n_rows < 0", who);
  a.theta = theta; a.X = X; a.n = n_rows; a.T = T; a.m2m = many_to_many ? 1 : 0;
  a.use_mask = a.m2m; a.mask_value = mask_value; a.out = out;
  return n_rows == 0;
}

// (the sign of the objective stays with the caller: VgArgs::negate, SVgArgs::sign)
template <class A, class LayFn>
static int lstm_value_grad_request(const char *who, A &a, LayFn lay, int n_models, const float *theta, const double *X,
                                   int64_t n_rows, int num_steps, int transform, float *val, double *grad) {
  if (const int rc = lstm_common(who, n_models, num_steps, lay)) return rc;
  if (!theta || !X || !val || !grad) return fail(BORE_E_INVALID, "%s: null pointer", who);
  if (const int rc = check_transform(who, transform)) return rc;
  if (n_rows < 0) return fail(BORE_E_INVALID, "%s: n_rows < 0", who);
  a.theta = theta; a.X = X; a.n = n_rows; a.T = num_steps; a.transform = transform; a.val = val; a.grad = grad;
  return n_rows == 0;
}

template <class A, class LayFn>
static int lstm_fit_request(const char *who, A &a, LayFn lay, int n_models, float *theta, float *adam_m, float *adam_v,
                            int64_t *adam_t, const float *X, const float *y, int64_t N, int T, float mask_value,
                            int epochs, int batch_size, const int32_t *perm, const bore_adam_cfg *adam,
                            float *epoch_loss) {
  if (const int rc = lstm_common(who, n_models, T, lay)) return rc;
  if (!theta || !adam_m || !adam_v || !adam_t || !X || !y || !adam) return fail(BORE_E_INVALID, "%s: null pointer", who);
  if (N < 1 || epochs < 0) return fail(BORE_E_INVALID, "%s: N must be >= 1 and epochs >= 0", who);
  if (batch_size < 1) return fail(BORE_E_INVALID, "%s: batch_size must be >= 1", who);
  if (batch_size > TILE)
    return fail(BORE_E_UNSUPPORTED, "%s: batch_size %d > %d (one tile of sequences per Adam step)", who, batch_size, TILE);
  if (epochs == 0) return 1;
  if (!perm) return fail(BORE_E_INVALID, "%s: explicit per-epoch permutations are required", who);
  if (N > 0x7fffffffLL) return fail(BORE_E_UNSUPPORTED, "%s: N > 2^31 - 1", who);
  a.theta = theta; a.am = adam_m; a.av = adam_v; a.at = (long long *)adam_t; a.X = X; a.Y = y; a.perm = perm;
  a.epoch_loss = epoch_loss; a.N = N; a.T = T; a.epochs = epochs; a.B = batch_size; a.mask_value = mask_value;
  a.lr = adam->lr; a.beta1 = adam->beta1; a.beta2 = adam->beta2; a.eps = adam->eps;
  return 0;
}

template <class A, class LayFn>
static int lstm_evaluate_request(const char *who, A &a, LayFn lay, int n_models, const float *theta, const float *X,
                                 const float *y, int64_t N, int T, float mask_value, float *loss, float *acc) {
  if (const int rc = lstm_common(who, n_models, T, lay)) return rc;
  if (!theta || !X || !y || !loss || !acc) return fail(BORE_E_INVALID, "%s: null pointer", who);
  if (N < 1) return fail(BORE_E_INVALID, "%s: N < 1", who);
  a.theta = theta; a.X = X; a.Y = y; a.N = N; a.T = T; a.mask_value = mask_value; a.loss = loss; a.acc = acc;
  return 0;
}

extern "C" int bore_lstm_forward(const bore_lstm_desc *desc, int n_models, const float *theta, const float *X,
                                 int64_t n_rows, int T, int many_to_many, float mask_value, float *out,
                                 void *stream) {
  FwdArgs A;
  int rc = lstm_forward_request("lstm_forward", A, [&] { return make_lay(desc, T, &A.a); }, n_models, theta, X, n_rows,
                                T, many_to_many, mask_value, out);
  if (rc) return rc < 0 ? rc : 0;
  const size_t bytes = (size_t)A.a.lds_floats * 4;
  rc = allow_lds(lstm_forward_kernel, bytes);
  if (rc) return rc;
  const long long tiles = (n_rows + TILE - 1) / TILE;
  if (tiles > 0x7fffffffLL) return fail(BORE_E_UNSUPPORTED, "lstm_forward: too many rows");
  hipLaunchKernelGGL(lstm_forward_kernel, dim3((unsigned)tiles, n_models), dim3(NT), bytes, (hipStream_t)stream, A);
  HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" int bore_lstm_value_and_input_grad(const bore_lstm_desc *desc, int n_models, const float *theta,
                                              const double *X, int64_t n_rows, int num_steps, int transform,
                                              int negate, float *val, double *grad, void *stream) {
  VgArgs A;
  int rc = lstm_value_grad_request("lstm_value_and_input_grad", A, [&] { return make_lay(desc, num_steps, &A.a); },
                                   n_models, theta, X, n_rows, num_steps, transform, val, grad);
  if (rc) return rc < 0 ? rc : 0;
  const long long tiles = (n_rows + TILE - 1) / TILE;
  if (tiles > 0x7fffffffLL) return fail(BORE_E_UNSUPPORTED, "lstm_value_and_input_grad: too many rows");
  A.negate = negate ? 1 : 0;
  const size_t bytes = (size_t)A.a.lds_floats * 4;
  rc = allow_lds(lstm_value_grad_kernel, bytes);
  if (rc) return rc;
  return with_workspace((size_t)n_models * tiles * A.a.ws_floats, stream, "lstm_value_grad_kernel", [&](float *ws) {
    A.ws = ws;
    hipLaunchKernelGGL(lstm_value_grad_kernel, dim3((unsigned)tiles, n_models), dim3(NT), bytes, (hipStream_t)stream, A);
    return 0;
  });
}

extern "C" int bore_lstm_fit(const bore_lstm_desc *desc, int n_models, float *theta, float *adam_m, float *adam_v,
                             int64_t *adam_t, const float *X, const float *y, int64_t N, int T, float mask_value,
                             int epochs, int batch_size, const int32_t *perm, const bore_adam_cfg *adam,
                             float *epoch_loss, void *stream) {
  FitArgsL A;
  int rc = lstm_fit_request("lstm_fit", A, [&] { return make_lay(desc, T, &A.a); }, n_models, theta, adam_m, adam_v,
                            adam_t, X, y, N, T, mask_value, epochs, batch_size, perm, adam, epoch_loss);
  if (rc) return rc < 0 ? rc : 0;
  const size_t bytes = (size_t)A.a.lds_floats * 4;
  rc = allow_lds(lstm_fit_kernel, bytes);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const size_t n_ws = (size_t)n_models * A.a.ws_floats, n_g = (size_t)n_models * A.a.P;
  return with_workspace(n_ws + n_g, stream, "lstm_fit", [&](float *buf) {
    A.ws = buf;
    A.gacc = buf + n_ws;
    const hipError_t e = hipMemsetAsync(A.gacc, 0, n_g * 4, st);
    if (e != hipSuccess) return fail(BORE_E_HIP, "lstm_fit: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(lstm_fit_kernel, dim3(n_models), dim3(NT), bytes, st, A);
    return 0;
  });
}

extern "C" int bore_lstm_evaluate(const bore_lstm_desc *desc, int n_models, const float *theta, const float *X,
                                  const float *y, int64_t N, int T, float mask_value, float *loss, float *acc,
                                  void *stream) {
  EvalArgsL A;
  int rc = lstm_evaluate_request("lstm_evaluate", A, [&] { return make_lay(desc, T, &A.a); }, n_models, theta, X, y, N,
                                 T, mask_value, loss, acc);
  if (rc) return rc;
  const size_t bytes = (size_t)A.a.lds_floats * 4;
  rc = allow_lds(lstm_evaluate_kernel, bytes);
  if (rc) return rc;
  hipLaunchKernelGGL(lstm_evaluate_kernel, dim3(n_models), dim3(NT), bytes, (hipStream_t)stream, A);
  HIP_TRY(hipGetLastError());
  return 0;
}
