// bore_ensemble.hip -- classifier ENSEMBLES: K members of one bore_mlp_desc, theta [n_ens][K][P], and an acquisition
// that reads all of them: the upper confidence bound s = mu + beta sigma of the members' outputs (the statement:
// bore_amd/ensemble.py, ensemble_score).  float32 networks, run-time layout only (the MlpLayout tables as the generic
// flavour uses them; no per-shape instantiation).  Entry points: bore_ensemble_value_and_input_grad,
// bore_ensemble_screen_topk, bore_ensemble_lbfgsb_minimize and the host query bore_ensemble_plan_query.
//
// One workgroup serves one ensemble and stages the K members' padded LDS images (load_theta) ONCE.  The unit of work
// is (row, member), done by ONE wave: units over lanes -- lane j forms unit j of a layer as one fmaf chain over the
// layer's inputs in ascending order (weights: consecutive lanes, consecutive banks; inputs: broadcast reads), the
// backward pass lane i the i-th input's delta as one fmaf chain over the layer's units.  The activations of the one
// row live in a per-wave strip of LDS; nothing of a row's arithmetic depends on which wave has it or on its
// neighbours: a row alone gives the bits it gives in a batch, an ensemble alone the bits it gives beside others.
// ensemble_pass -- up to ENS_ROWS rows x K members dealt over the four waves, then the float64 combination, one
// wave per row -- is the ONE definition behind the public value + gradient entry point and the `pass` that
// stream_restart_drive (bore_stream.hip) runs per round of the restarts: the two agree bit for bit.  The pass is
// latency-bound (a few rows, tiny products); profiles/ensemble/ holds what was measured.  No float atomics, no
// workgroup waits for another.
#include <hip/hip_runtime.h>

#include <cmath>

#include "host_common.h"
#include "lbfgsb.h"
#include "mlp_device.h"
#include "mlp_math.h"
#include "stream_restart.h"

namespace bore {

constexpr int ENS_ROWS = BORE_THREADS / 64;  // rows of a pass: one per wave in the combination and in the restarts

// Float offsets from the 16-byte aligned start of the ensemble's LDS region, every region a multiple of 16 bytes:
// layout | pre (where A_l sits in a wave's strip; [0]: the widest layer) | K padded images of theta | x: ENS_ROWS
// points [D] | per wave a strip of wave_floats: A_1..A_n of its row, two delta buffers | F [K][ENS_ROWS] | G
// [K][ENS_ROWS][D] | val [ENS_ROWS] | grad fp64 [ENS_ROWS][D].
struct EnsCarve {
  int o_layout, o_pre, o_theta, o_x, o_wave, wave_floats, o_f, o_g, o_val, o_grad, total;
};

struct EnsArgs {
  MlpLayout L;
  EnsCarve c;
  const float *theta;  // [n_ens][K][P]
  int K;
  double beta;
};

struct EnsView {
  const MlpLayout *L;
  const int *pre;
  const float *theta;
  float *x, *wave, *F, *G, *val;
  double *grad;
  int K, wave_floats;
};

__device__ __forceinline__ float *ensemble_dyn(float *smem) {
  return reinterpret_cast<float *>(reinterpret_cast<char *>(smem) + ((16 - ((size_t)smem & 15)) & 15));
}

// Start of every ensemble kernel: zero the region, park the layout and the strip offsets, stage the K images of
// ensemble `ens`.  Called by the whole workgroup; ends with a barrier.
__device__ __forceinline__ EnsView ensemble_begin(float *base, const EnsArgs &a, const long long ens) {
  const int tid = threadIdx.x, nthr = blockDim.x;
  for (int i = tid; i < a.c.total; i += nthr) base[i] = 0.f;
  __syncthreads();
  const int *src = reinterpret_cast<const int *>(&a.L);
  int *dst = reinterpret_cast<int *>(base + a.c.o_layout);
  for (int i = tid; i < (int)(sizeof(MlpLayout) / 4); i += nthr) dst[i] = src[i];
  int *pre = reinterpret_cast<int *>(base + a.c.o_pre);
  if (tid == 0) {
    int s = 0, maxw = 1;
    for (int l = 1; l <= a.L.n_layers; ++l) {
      pre[l] = s;
      s += a.L.w[l];
      maxw = a.L.w[l] > maxw ? a.L.w[l] : maxw;
    }
    pre[a.L.n_layers + 1] = s;  // the two delta buffers: [maxw] each
    pre[0] = maxw;
  }
  __syncthreads();
  EnsView E;
  E.L = reinterpret_cast<const MlpLayout *>(base + a.c.o_layout);
  E.pre = pre;
  E.theta = base + a.c.o_theta;
  E.x = base + a.c.o_x;
  E.wave = base + a.c.o_wave;
  E.F = base + a.c.o_f;
  E.G = base + a.c.o_g;
  E.val = base + a.c.o_val;
  E.grad = reinterpret_cast<double *>(base + a.c.o_grad);
  E.K = a.K;
  E.wave_floats = a.c.wave_floats;
  const MlpLayout &L = *E.L;
  const float *th = a.theta + ens * a.K * L.P;
  for (int k = 0; k < a.K; ++k) load_theta(L, L.n_layers, th + (long long)k * L.P, base + a.c.o_theta + k * L.P_lds);
  __syncthreads();
  return E;
}

// One member's forward pass of one row, by the calling wave: x [D] (LDS) -> A_l at act + pre[l], l = 1..n; returns
// f = A_n[0].  th: the member's padded image.
__device__ __forceinline__ float ensemble_member_forward(const EnsView &E, const float *th, const float *x, float *act) {
  const MlpLayout &L = *E.L;
  const int lane = threadIdx.x & 63, n = L.n_layers;
  const float *in = x;
  for (int l = 1; l <= n; ++l) {
    const float *W = th + L.woff[l], *bias = th + L.boff[l];
    const int ldw = L.ldw[l], kin = L.w[l - 1], nout = L.w[l], a = L.act[l];
    float *out = act + E.pre[l];
    for (int j = lane; j < nout; j += 64) {
      float acc = 0.f;
      for (int k = 0; k < kin; ++k) acc = fmaf(in[k], W[k * ldw + j], acc);
      out[j] = act_fwd<false>(a, acc + bias[j]);
    }
    wave_lds_sync();
    in = out;
  }
  return in[0];
}

// The same member's input gradient of f, by the calling wave behind its forward pass: g [D] (LDS).
__device__ __forceinline__ void ensemble_member_backward(const EnsView &E, const float *th, const float *act,
                                                         float *dbuf, const float f, float *g) {
  const MlpLayout &L = *E.L;
  const int lane = threadIdx.x & 63, n = L.n_layers;
  float *din = dbuf, *dout = dbuf + E.pre[0];
  if (lane == 0) din[0] = act_grad(L.act[n], f);
  wave_lds_sync();
  for (int l = n; l >= 1; --l) {
    const float *W = th + L.woff[l];
    const int ldw = L.ldw[l], kin = L.w[l - 1], nout = L.w[l], a = L.act[l - 1];
    const float *aprev = act + E.pre[l - 1];  // (l == 1: not read)
    float *o = l > 1 ? dout : g;
    for (int i = lane; i < kin; i += 64) {
      float acc = 0.f;
      for (int j = 0; j < nout; ++j) acc = fmaf(din[j], W[i * ldw + j], acc);
      if (l > 1) acc *= act_grad(a, aprev[i]);
      o[i] = acc;
    }
    wave_lds_sync();
    float *t = din;
    din = dout;
    dout = t;
  }
}

// mu and sigma of K outputs F[k * stride], float64, sums in the order k = 0 .. K - 1 (bore_amd/ensemble.py).
__device__ __forceinline__ void ensemble_mu_sigma(const float *F, const int stride, const int K, double &mu, double &sigma) {
  double sum = 0.0;
  for (int k = 0; k < K; ++k) sum += (double)F[k * stride];
  mu = sum / (double)K;
  double v = 0.0;
  for (int k = 0; k < K; ++k) {
    const double d = (double)F[k * stride] - mu;
    v += d * d;
  }
  sigma = sqrt(v / (double)K + BORE_ENSEMBLE_VAR_FLOOR);
}

// Value and input gradient of T(sign s), s = mu + beta sigma, for the nr <= ENS_ROWS rows whose points sit in E.x:
// f_k and grad f_k of every (row, member) into F and G, the pairs dealt over the waves; then wave r combines row r in
// float64 -- val[r] = T(float32(sign s)), grad[r] = sign T' sum_k c_k grad f_k, c_k = 1/K + beta d_k / (K sigma).
// Called by the whole workgroup after a barrier behind the writes of E.x; ends with a barrier, after which val and
// grad are visible to every wave.
__device__ __forceinline__ void ensemble_pass(const EnsView &E, const int nr, const double beta, const int transform,
                                              const float sign) {
  const MlpLayout &L = *E.L;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const int K = E.K, D = L.w[0], n = L.n_layers;
  float *act = E.wave + wv * E.wave_floats;
  for (int t = wv; t < nr * K; t += ENS_ROWS) {
    const int r = t / K, k = t - r * K;
    const float *th = E.theta + k * L.P_lds;
    const float f = ensemble_member_forward(E, th, E.x + r * D, act);
    if (lane == 0) E.F[k * ENS_ROWS + r] = f;
    ensemble_member_backward(E, th, act, act + E.pre[n + 1], f, E.G + (k * ENS_ROWS + r) * D);
  }
  __syncthreads();
  if (wv < nr) {
    const int r = wv;
    double mu, sigma;
    ensemble_mu_sigma(E.F + r, ENS_ROWS, K, mu, sigma);
    const double s = mu + beta * sigma;
    float T, dT;
    objective_transform(transform, sign * (float)s, T, dT);
    const double gs = (double)(sign * dT);
    for (int d = lane; d < D; d += 64) {
      double acc = 0.0;
      for (int k = 0; k < K; ++k) {
        const double dk = (double)E.F[k * ENS_ROWS + r] - mu;
        const double ck = 1.0 / (double)K + beta * dk / ((double)K * sigma);
        acc += ck * (double)E.G[(k * ENS_ROWS + r) * D + d];
      }
      E.grad[r * D + d] = gs * acc;
    }
    if (lane == 0) E.val[r] = T;
  }
  __syncthreads();
}

// ---- value + input gradient: grid (ensemble, walkers over the tiles of ENS_ROWS rows) ----
struct EnsRowArgs {
  EnsArgs e;
  const double *X;
  float *val;
  double *grad;
  long long n_rows;
  int transform;
  float sign;
};

__global__ __launch_bounds__(BORE_THREADS) void ensemble_rows_kernel(const EnsRowArgs a) {
  extern __shared__ float smem[];
  const long long ens = blockIdx.x;
  const EnsView E = ensemble_begin(ensemble_dyn(smem), a.e, ens);
  const int tid = threadIdx.x, D = E.L->w[0];
  const long long n_tiles = (a.n_rows + ENS_ROWS - 1) / ENS_ROWS;
  for (long long t = blockIdx.y; t < n_tiles; t += gridDim.y) {
    const long long row0 = ens * a.n_rows + t * ENS_ROWS;
    const int nr = (int)min((long long)ENS_ROWS, a.n_rows - t * ENS_ROWS);
    for (int i = tid; i < nr * D; i += BORE_THREADS) E.x[i] = (float)a.X[row0 * D + i];  // Keras autocast fp64 -> fp32
    __syncthreads();
    ensemble_pass(E, nr, a.e.beta, a.transform, a.sign);
    for (int i = tid; i < nr * D; i += BORE_THREADS) a.grad[row0 * D + i] = E.grad[i];
    if (tid < nr) a.val[row0 + tid] = E.val[tid];
    __syncthreads();  // (the next tile overwrites x, val and grad)
  }
}

// ---- screening: s of every candidate, a wave per row with the K loop inside; the selection is the library's
// stream_select_kernel (bore_stream.hip), which ranks a score buffer and never looks at a network ----
struct EnsScoreArgs {
  EnsArgs e;
  const double *X;
  float *score;
  long long n_samples;
  int x_shared;
};

__global__ __launch_bounds__(BORE_THREADS) void ensemble_score_kernel(const EnsScoreArgs a) {
  extern __shared__ float smem[];
  const long long ens = blockIdx.x;
  const EnsView E = ensemble_begin(ensemble_dyn(smem), a.e, ens);
  const MlpLayout &L = *E.L;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const int K = E.K, D = L.w[0];
  float *act = E.wave + wv * E.wave_floats, *xrow = E.x + wv * D;
  const double *X = a.X + (a.x_shared ? 0 : ens * a.n_samples * D);
  for (long long r = (long long)blockIdx.y * ENS_ROWS + wv; r < a.n_samples; r += (long long)gridDim.y * ENS_ROWS) {
    for (int d = lane; d < D; d += 64) xrow[d] = (float)X[r * D + d];  // Keras autocast fp64 -> fp32
    wave_lds_sync();
    for (int k = 0; k < K; ++k) {
      const float f = ensemble_member_forward(E, E.theta + k * L.P_lds, xrow, act);
      if (lane == 0) E.F[k * ENS_ROWS + wv] = f;
    }
    wave_lds_sync();
    double mu, sigma;
    ensemble_mu_sigma(E.F + wv, ENS_ROWS, K, mu, sigma);
    if (lane == 0) a.score[ens * a.n_samples + r] = (float)(mu + a.e.beta * sigma);
    wave_lds_sync();  // (the next row overwrites F)
  }
}

// ---- restarts: stream_restart_drive around ensemble_pass.  The driver's carve (stream_restart.h) comes first in the
// dynamic LDS, the ensemble's region behind it at float offset ens_base. ----
struct EnsLbfgsbArgs {
  EnsArgs e;
  int ens_base;
  RestartArgs r;
};

__global__ __launch_bounds__(BORE_THREADS) void ensemble_lbfgsb_kernel(const EnsLbfgsbArgs a) {
  extern __shared__ float smem[];
  const EnsView E = ensemble_begin(ensemble_dyn(smem) + a.ens_base, a.e, blockIdx.x);
  const int D = E.L->w[0];
  stream_restart_drive(
      a.r, D, [] {},  // (rows of waves that never ask: zeros, from ensemble_begin)
      [&](const int wv, const int lane, const double *x) {
        for (int d = lane; d < D; d += 64) E.x[wv * D + d] = (float)x[d];  // Keras autocast fp64 -> fp32
      },
      [&] { ensemble_pass(E, ENS_ROWS, a.e.beta, a.r.transform, a.r.sign); },
      [&](const int wv, const int lane, double &f, double *g) {
        f = (double)E.val[wv];
        for (int d = lane; d < D; d += 64) g[d] = E.grad[wv * D + d];
      });
}

}  // namespace bore

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
using namespace bore;

// What a request of these sizes would launch: the ensemble's region, and -- maxcor > 0 -- the restart driver's carve
// in front of it.  Sizes in bytes as 64-bit values: a refusal names them whatever they are.
struct EnsPlan {
  EnsCarve c;
  long long image_bytes, pass_bytes, region_bytes;  // K images | the rest of the region | both
  RestartCarve rc;                                  // (maxcor > 0)
  long long lds_bytes;                              // the launch's dynamic LDS
  int ens_base;
};

// The bounds every ensemble entry point shares, each refused by name, in this order, before any HIP call: the
// descriptor, n_ens, K, compute, the last layer, beta, the LDS of the images and the pass.  Behind it, in the entry
// points: (restarts) the options and the box, then ensemble_restart_plan -- the LDS of the restart slots -- and last
// ensemble_no_batch.
static int ensemble_plan(const char *who, const bore_mlp_desc *desc, int n_ens, int K, double beta, EnsArgs *a,
                         EnsPlan *p) {
  if (!desc) return fail(BORE_E_INVALID, "%s: null pointer", who);
  MlpLayout &L = a->L;
  if (bore_make_layout(desc, 0, ENS_ROWS, &L)) return fail(BORE_E_INVALID, "bad bore_mlp_desc");
  if (n_ens < 1 || n_ens > 65535) return fail(BORE_E_INVALID, "%s: n_ensembles must be 1..65535 (got %d)", who, n_ens);
  if (K < 1 || K > BORE_ENSEMBLE_MAX_MEMBERS)
    return fail(BORE_E_UNSUPPORTED, "%s: an ensemble has 1..%d members (BORE_ENSEMBLE_MAX_MEMBERS), got %d", who,
                BORE_ENSEMBLE_MAX_MEMBERS, K);
  if (desc->compute != BORE_COMPUTE_F32)
    return fail(BORE_E_UNSUPPORTED, "%s: the ensemble kernels take compute = float32 members only", who);
  if (L.w[L.n_layers] != 1) return fail(BORE_E_INVALID, "%s: the last Dense layer must have 1 unit", who);
  if (!(beta >= 0.0) || !std::isfinite(beta))
    return fail(BORE_E_INVALID, "%s: beta must be finite and >= 0 (got %g)", who, beta);
  const int D = L.w[0];
  auto up4 = [](long long v) { return (v + 3) & ~3ll; };
  long long sumw = 0, maxw = 1;
  for (int l = 1; l <= L.n_layers; ++l) {
    sumw += L.w[l];
    maxw = L.w[l] > maxw ? L.w[l] : maxw;
  }
  const long long wave_floats = up4(sumw + 2 * maxw);
  long long off = 0, o[10];
  o[0] = off; off += BORE_LAYOUT_FLOATS;
  o[1] = off; off += up4(BORE_MAX_LAYERS + 2);
  o[2] = off; off += up4((long long)K * L.P_lds);
  o[3] = off; off += up4((long long)ENS_ROWS * D);
  o[4] = off; off += ENS_ROWS * wave_floats;
  o[5] = off; off += up4((long long)K * ENS_ROWS);
  o[6] = off; off += up4((long long)K * ENS_ROWS * D);
  o[7] = off; off += 4;
  o[8] = off; off += 2 * up4((long long)ENS_ROWS * D);
  p->image_bytes = 4 * up4((long long)K * L.P_lds);
  p->region_bytes = 4 * off;
  p->pass_bytes = p->region_bytes - p->image_bytes;
  if (p->region_bytes + 16 > BORE_LDS_BYTES)
    return fail(BORE_E_UNSUPPORTED,
                "%s: %d members' images (%lld B) plus the pass workspace (%lld B) need %lld B of LDS (> %d): fewer "
                "members, or a smaller network", who, K, p->image_bytes, p->pass_bytes, p->region_bytes + 16,
                BORE_LDS_BYTES);
  a->c = EnsCarve{(int)o[0], (int)o[1], (int)o[2], (int)o[3], (int)o[4], (int)wave_floats,
                  (int)o[5], (int)o[6], (int)o[7], (int)o[8], (int)off};
  p->c = a->c;
  p->ens_base = 0;
  p->lds_bytes = p->region_bytes + 16;
  p->rc = RestartCarve{};
  a->K = K;
  a->beta = beta;
  return 0;
}

// The restart driver's carve (stream_restart.h) in front of the region ensemble_plan laid out.
static int ensemble_restart_plan(const char *who, const EnsArgs &a, int maxcor, EnsPlan *p) {
  static_assert(STREAM_RESTART_LDS_BYTES == BORE_LDS_BYTES, "stream_restart.h carves another LDS");
  const int D = a.L.w[0];
  if (D > BORE_DIM_MAX)
    return fail(BORE_E_UNSUPPORTED, "%s: the restarts take D <= BORE_DIM_MAX = %d (got %d)", who, BORE_DIM_MAX, D);
  if (maxcor < 1 || maxcor > 32) return fail(BORE_E_UNSUPPORTED, "lbfgsb_minimize: maxcor must be 1..32");
  if (!stream_restart_carve(D, maxcor, (size_t)p->region_bytes, ENS_ROWS, &p->rc))
    return fail(BORE_E_UNSUPPORTED,
                "%s: %d members' images (%lld B) plus the pass workspace (%lld B) leave %zu B of LDS (of %d) for the "
                "restart slots, one needs %zu B at D = %d, maxcor = %d: fewer members, or lower maxcor", who, a.K,
                p->image_bytes, p->pass_bytes, p->rc.room, BORE_LDS_BYTES, (size_t)p->rc.lds.prob_floats * 4, D, maxcor);
  p->ens_base = (int)(((p->rc.lds_bytes - 16) / 4 + 3) & ~(size_t)3);  // (behind the slots, on a 16-byte boundary)
  p->lds_bytes = 4ll * p->ens_base + 16 + p->region_bytes;
  return 0;
}

static int ensemble_no_batch(const char *who, bool batch) {
  if (batch) return fail(BORE_E_UNSUPPORTED, "%s: batch mode (bore_set_batch) takes no ensembles", who);
  return 0;
}

// Workgroups per ensemble over `units` units of work: two per CU's worth over the ensembles, <= 65535, >= 1.
static unsigned ensemble_walkers(int n_ens, long long units) {
  long long gy = units;
  const long long cap = (2 * device_cus() + n_ens - 1) / n_ens;
  if (gy > cap) gy = cap;
  if (gy > 65535) gy = 65535;
  return (unsigned)(gy < 1 ? 1 : gy);
}

extern "C" int bore_ensemble_plan_query(const bore_mlp_desc *desc, int n_ens, int K, double beta, int maxcor,
                                        int batch_mode, int32_t *out, int n_out) {
  static const char who[] = "ensemble_plan_query";
  if (!desc || !out) return fail(BORE_E_INVALID, "%s: null pointer", who);
  if (n_out < BORE_ENSEMBLE_PLAN_FIELDS)
    return fail(BORE_E_INVALID, "%s: out holds fewer than %d fields", who, BORE_ENSEMBLE_PLAN_FIELDS);
  EnsArgs a;
  EnsPlan p;
  if (const int rc = ensemble_plan(who, desc, n_ens, K, beta, &a, &p)) return rc;
  if (maxcor != 0)  // (0: the value + gradient and screening kernels, which carve no restart slots)
    if (const int rc = ensemble_restart_plan(who, a, maxcor, &p)) return rc;
  if (const int rc = ensemble_no_batch(who, batch_mode != 0 || g_batch)) return rc;
  const long long fields[BORE_ENSEMBLE_PLAN_FIELDS] = {
      K, a.L.P_lds, p.image_bytes, p.pass_bytes, p.lds_bytes, p.rc.waves, (long long)p.rc.lds.prob_floats * 4,
      p.ens_base, a.c.o_layout, a.c.o_pre, a.c.o_theta, a.c.o_x, a.c.o_wave, a.c.wave_floats, a.c.o_f, a.c.o_g,
      a.c.o_val, a.c.o_grad, a.c.total, p.rc.lds.o_box, p.rc.lds.o_vote, p.rc.lds.o_prob, p.rc.lds.o_dw, p.rc.lds.o_iw};
  for (int i = 0; i < BORE_ENSEMBLE_PLAN_FIELDS; ++i) out[i] = (int32_t)fields[i];
  return 0;
}

extern "C" int bore_ensemble_value_and_input_grad(const bore_mlp_desc *desc, int n_ens, int K, const float *theta,
                                                  const double *X, int64_t n_rows, double beta, int transform,
                                                  int negate, float *val, double *grad, void *stream) {
  static const char who[] = "ensemble_value_and_input_grad";
  EnsRowArgs a;
  EnsPlan p;
  if (const int rc = ensemble_plan(who, desc, n_ens, K, beta, &a.e, &p)) return rc;
  if (const int rc = check_transform(who, transform)) return rc;
  if (!theta || !X || !val || !grad) return fail(BORE_E_INVALID, "%s: null pointer", who);
  if (n_rows < 0) return fail(BORE_E_INVALID, "%s: n_rows < 0", who);
  if (const int rc = ensemble_no_batch(who, g_batch != nullptr)) return rc;
  if (n_rows == 0) return 0;
  a.e.theta = theta; a.X = X; a.val = val; a.grad = grad;
  a.n_rows = n_rows; a.transform = transform; a.sign = negate ? -1.f : 1.f;
  const unsigned gy = ensemble_walkers(n_ens, (n_rows + ENS_ROWS - 1) / ENS_ROWS);
  return launch_lds(ensemble_rows_kernel, dim3(n_ens, gy), dim3(BORE_THREADS), (size_t)p.lds_bytes, stream, a);
}

extern "C" int bore_ensemble_screen_topk(const bore_mlp_desc *desc, int n_ens, int K, const float *theta,
                                         const double *X_init, int64_t n_samples, int x_shared, double beta,
                                         int num_starts, double *x0, int32_t *idx, float *score, void *stream) {
  static const char who[] = "ensemble_screen_topk";
  EnsScoreArgs a;
  EnsPlan p;
  if (const int rc = ensemble_plan(who, desc, n_ens, K, beta, &a.e, &p)) return rc;
  if (!theta || !X_init || !x0 || !idx) return fail(BORE_E_INVALID, "%s: null pointer", who);
  if (n_samples < 1) return fail(BORE_E_INVALID, "%s: n_samples out of range", who);
  if (num_starts < 1 || num_starts > n_samples) return fail(BORE_E_INVALID, "%s: need 1 <= num_starts <= n_samples", who);
  if (n_samples > BORE_STREAM_MAX_SAMPLES)
    return fail(BORE_E_UNSUPPORTED,
                "%s: the selection ranks n_samples <= BORE_STREAM_MAX_SAMPLES = %d sort keys in one workgroup's LDS "
                "(got %lld)", who, BORE_STREAM_MAX_SAMPLES, (long long)n_samples);
  if (const int rc = ensemble_no_batch(who, g_batch != nullptr)) return rc;
  a.e.theta = theta; a.X = X_init; a.n_samples = n_samples; a.x_shared = x_shared;
  int n_pad = 1;
  while (n_pad < n_samples) n_pad <<= 1;
  StreamSampleArgs sp{};  // (candidates in memory: no sampled form)
  StreamSelectArgs sel;
  sel.X = X_init; sel.x0 = x0; sel.idx = idx;
  sel.n_samples = n_samples; sel.x_shared = x_shared; sel.R = num_starts; sel.n_pad = n_pad; sel.D = a.e.L.w[0];
  const size_t key_bytes = 8 * ((size_t)n_pad + 32) + 8;
  // (a workgroup stages the K images once: at least 16 rows each, 4 per wave)
  const unsigned gy = ensemble_walkers(n_ens, (n_samples + 4 * ENS_ROWS - 1) / (4 * ENS_ROWS));
  auto run = [&](float *buf) {
    a.score = buf;
    sel.pred = buf;
    if (const int rc = allow_lds(stream_select_kernel, key_bytes)) return rc;
    if (const int rc = launch_lds(ensemble_score_kernel, dim3(n_ens, gy), dim3(BORE_THREADS), (size_t)p.lds_bytes, stream, a))
      return rc;
    hipLaunchKernelGGL(stream_select_kernel, dim3(n_ens), dim3(BORE_THREADS), key_bytes, (hipStream_t)stream, sel, sp);
    HIP_TRY(hipGetLastError());
    return 0;
  };
  if (score) return run(score);
  return with_workspace((size_t)n_ens * n_samples, stream, "ensemble screening", run);
}

extern "C" int bore_ensemble_lbfgsb_minimize(const bore_mlp_desc *desc, int n_ens, int K, const float *theta, double beta,
                                             int transform, int negate, const double *x0, int num_starts,
                                             const double *lb, const double *ub, const bore_lbfgsb_opts *opts,
                                             double *x, double *fun, double *jac, int32_t *info, void *stream) {
  static const char who[] = "ensemble_lbfgsb_minimize";
  EnsLbfgsbArgs a;
  EnsPlan p;
  if (const int rc = ensemble_plan(who, desc, n_ens, K, beta, &a.e, &p)) return rc;
  RestartArgs &r = a.r;
  if (const int rc = lbfgsb_check_args(LbfgsbRequest{desc, n_ens, theta, transform, negate, x0, num_starts, lb, ub, opts,
                                                     x, fun, jac, info}, r.box, r.nbd, r.opt))
    return rc;
  if (const int rc = ensemble_restart_plan(who, a.e, r.opt.m, &p)) return rc;
  if (const int rc = ensemble_no_batch(who, g_batch != nullptr)) return rc;
  a.e.theta = theta;
  a.ens_base = p.ens_base;
  r.x0 = x0; r.x = x; r.fun = fun; r.jac = jac; r.info = info;
  r.R = num_starts; r.transform = transform; r.sign = negate ? -1.f : 1.f;
  r.lds = p.rc.lds;
  r.waves = p.rc.waves;
  r.ws = nullptr;  // (everything of the pass lives in LDS)
  r.ws_stride = 0;
  // a workgroup per group of `waves` restarts; beyond the grid's 65535 a workgroup walks several groups
  const long long groups = ((long long)num_starts + r.waves - 1) / r.waves;
  const long long gy = groups > 65535 ? 65535 : groups;
  r.max_rounds = ((groups + gy - 1) / gy) * lbfgsb_round_cap(opts);
  return launch_lds(ensemble_lbfgsb_kernel, dim3(n_ens, (unsigned)gy), dim3(BORE_THREADS), (size_t)p.lds_bytes, stream, a);
}
