// stream_restart.h -- the dynamic-LDS carve of the streamed restart kernels (stream_restart_drive in bore_stream.hip:
// stream_lbfgsb_kernel and lstm_stream_lbfgsb_kernel).  Host code over lbfgsb.h and plain integers, so that the host
// build of the tests (tests/native/lbfgsb_host.cpp) states the very carve the entry points launch with.
#pragma once
#include <stddef.h>

#include "lbfgsb.h"

constexpr size_t STREAM_RESTART_LDS_BYTES = 160 * 1024;  // one workgroup's LDS (BORE_LDS_BYTES: bore_stream.hip asserts it)
// beside the kernel's static LDS: its own alignment and the 16 bytes the driver may skip to align the dynamic region
constexpr size_t STREAM_RESTART_SLACK = 64;

// Float offsets from the 16-byte aligned start of the dynamic LDS: box (lo, hi: De doubles each; nbd) | vote (4 ints)
// | per wave a slot of prob_floats: the parked State, at o_dw the optimiser's fp64 workspace, at o_iw its int one.
// Every region a multiple of 16 bytes (fp64 LDS reads merge into ds_read_b128; a slot is zeroed as float4).
struct RestartLds {
  int o_box, o_vote, o_prob, prob_floats, o_dw, o_iw;
};

struct RestartCarve {
  RestartLds lds;
  int waves;         // how many waves hold a problem: the slots that fit, at most max_waves; 0: not even one
  size_t lds_bytes;  // of the launch's dynamic LDS
  size_t room;       // bytes there are for the slots
};

// The carve for D variables and `maxcor` corrections beside `static_bytes` of static LDS.  False: no room for one slot
// (c->lds.prob_floats and c->room say how far off).
inline bool stream_restart_carve(int D, int maxcor, size_t static_bytes, int max_waves, RestartCarve *c) {
  const int De = (D + 1) & ~1;
  size_t off = 0;
  c->lds.o_box = 0; off += 4 * (size_t)De + (((size_t)D + 3) & ~(size_t)3);
  c->lds.o_vote = (int)off; off += 4;
  c->lds.o_prob = (int)off;
  const size_t state_f = (sizeof(lbfgsb::State) + 15) / 16 * 4;
  const size_t dw_f = 2 * (size_t)lbfgsb::dwork_size(D, maxcor);
  const size_t iw_f = ((size_t)lbfgsb::iwork_size(D) + 3) & ~(size_t)3;
  c->lds.o_dw = (int)state_f;
  c->lds.o_iw = (int)(state_f + dw_f);
  c->lds.prob_floats = (int)(state_f + dw_f + iw_f);
  const size_t taken = static_bytes + STREAM_RESTART_SLACK + off * 4;
  c->room = taken < STREAM_RESTART_LDS_BYTES ? STREAM_RESTART_LDS_BYTES - taken : 0;
  const size_t fit = c->room / ((size_t)c->lds.prob_floats * 4);
  c->waves = fit < (size_t)max_waves ? (int)fit : max_waves;
  c->lds_bytes = (off + (size_t)c->waves * c->lds.prob_floats) * 4 + 16;
  return c->waves >= 1;
}
