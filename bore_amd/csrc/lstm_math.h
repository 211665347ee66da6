// lstm_math.h -- the scalar arithmetic of an LSTM cell and of its masked loss, each formula defined once for the
// two flavours of the recurrent classifier (bore_lstm.hip: LDS, bore_lstm_stream.hip: streamed), as mlp_math.h
// does for the Dense kernels.  Device-only, IEEE forms throughout; under -ffp-contract=off the order of the
// operations below IS the rounding.  What is NOT here: the one line that forms c from the gates -- the flavours
// round it differently and each keeps its own.
#pragma once
#include "mlp_math.h"

namespace bore_lstm {

using bore::sigmoid_stable, bore::act_grad, bore::bce_loss, bore::accuracy_hit;

// act(x); elu through expm1f for x <= 0, NaN in -> NaN out (act_fwd's ReLU, fmaxf, gives 0 for NaN: not the same function)
__device__ __forceinline__ float actf(int a, float x) {
  switch (a) {
    case BORE_ACT_RELU: return x > 0.f ? x : (x == x ? 0.f : x);
    case BORE_ACT_ELU: return x > 0.f ? x : expm1f(x);
    case BORE_ACT_SIGMOID: return sigmoid_stable(x);
    case BORE_ACT_TANH: return tanhf(x);
    default: return x;
  }
}

// input, forget, candidate and output gate of one unit (Keras order i, f, c, o), from its four pre-activations
struct Gates { float i, f, g, o; };
__device__ __forceinline__ Gates gates_of(int act, float zi, float zf, float zg, float zo) {
  return Gates{sigmoid_stable(zi), sigmoid_stable(zf), actf(act, zg), sigmoid_stable(zo)};
}

// h = o act(c) of the new c, and what the step leaves behind: a masked step keeps the (cp, hp) it found
__device__ __forceinline__ void cell_out(int act, float go, float c, float cp, float hp, bool live, float &cn, float &hn) {
  const float h = go * actf(act, c);
  cn = live ? c : cp;
  hn = live ? h : hp;
}

// Deltas of the four pre-activations (0 on a masked step) and of c as handed to the step before (a masked step hands
// on what it got), from the gates and c of the step, c of the step before, and the deltas dh, dc_in of h and c.
struct GateDeltas { float zi, zf, zg, zo, c; };
__device__ __forceinline__ GateDeltas gate_deltas(int act, const Gates &g, float c, float cp, float dh, float dc_in,
                                                  bool live) {
  const float ac = actf(act, c);
  const float dct = dc_in + dh * g.o * act_grad(act, ac);
  const float dzi = dct * g.g * (g.i * (1.f - g.i));
  const float dzf = dct * cp * (g.f * (1.f - g.f));
  const float dzg = dct * g.i * act_grad(act, g.g);
  const float dzo = dh * ac * (g.o * (1.f - g.o));
  return GateDeltas{live ? dzi : 0.f, live ? dzf : 0.f, live ? dzg : 0.f, live ? dzo : 0.f, live ? dct * g.f : dc_in};
}

// One (sequence, step) element of the masked BCE from the logit x: returns its loss term, dlogit = its delta,
// (sigmoid(x) - y) scale; both 0 where the step is masked.
__device__ __forceinline__ float masked_bce(float x, float y, bool live, float scale, float &dlogit) {
  const float l = bce_loss(x, y);
  dlogit = live ? (sigmoid_stable(x) - y) * scale : 0.f;
  return live ? l : 0.f;
}

// ... and of the masked binary_accuracy on the model output (the logit) at 0.5: adds to the hits and to the live count
__device__ __forceinline__ void masked_hit(float x, float y, bool live, float &hits, float &n) {
  hits += live ? accuracy_hit(x, y) : 0.f;
  n += live ? 1.f : 0.f;
}

// pen + f w^2: the l2 penalty of one parameter with factor f, added to a running sum
__device__ __forceinline__ float l2_term(float f, float w, float pen) { return fmaf(f * w, w, pen); }

}  // namespace bore_lstm
