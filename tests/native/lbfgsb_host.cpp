// Host build of bore_amd/csrc/lbfgsb.h (the L-BFGS-B state machine that runs inside the
// HIP argmax kernel) so that it can be driven from pytest on a machine without a GPU.
// f/g come from a Python callback.  Test scaffolding only.
#include <cstdlib>
#include <vector>

// The events of lbfgsb.h (EV_*: bound kinds met, recovery branches taken) are counted here, per thread, and handed out
// by lbfgsb_host_minimize_events; counting touches nothing the optimiser reads.
#define LBFGSB_HOST_EVENTS
static thread_local int lbfgsb_host_events[32];
#define LB_EVENT(s_, id) ((void)++lbfgsb_host_events[id])

#include "../../bore_amd/csrc/lbfgsb.h"
#include "../../bore_amd/csrc/stream_restart.h"

static_assert(lbfgsb::EV_COUNT <= 32, "lbfgsb_host_events is too short");

extern "C" {

// stream_restart_carve, the carve the streamed restart entry points launch with: out = {o_box, o_vote, o_prob,
// prob_floats, o_dw, o_iw, waves, lds_bytes, room}; sizes = {sizeof(State), dwork_size, iwork_size}.  Returns 1 when a
// slot fits, else 0.
int lbfgsb_host_stream_restart_carve(int D, int maxcor, long long static_bytes, int max_waves, long long *out,
                                     int *sizes) {
  RestartCarve c;
  const bool fits = stream_restart_carve(D, maxcor, (size_t)static_bytes, max_waves, &c);
  const long long v[9] = {c.lds.o_box, c.lds.o_vote, c.lds.o_prob, c.lds.prob_floats, c.lds.o_dw,
                          c.lds.o_iw,  c.waves,      (long long)c.lds_bytes, (long long)c.room};
  for (int i = 0; i < 9; ++i) out[i] = v[i];
  sizes[0] = (int)sizeof(lbfgsb::State);
  sizes[1] = lbfgsb::dwork_size(D, maxcor);
  sizes[2] = lbfgsb::iwork_size(D);
  return fits ? 1 : 0;
}

typedef void (*fg_callback)(int n, const double *x, double *f, double *g);

// Returns the number of evaluations asked of the callback.  out_i = {nit, nfev, status, task, msg}.
// form 0: reverse communication (lbfgsb_advance returns for every evaluation); 1: the DIRECT form
// (the routine calls the evaluation); 2: DIRECT with the two-variable line search in registers
// (n == 2; other n fall back to form 1 inside the routine).
int lbfgsb_host_minimize_form(int form, int n, int m, const double *x0, const double *l, const double *u,
                              const int *nbd, double factr, double pgtol, int maxiter, int maxfun,
                              int maxls, fg_callback fg, double *x_out, double *f_out, double *g_out,
                              int *out_i) {
  using namespace lbfgsb;
  std::vector<double> dw(dwork_size(n, m), 0.0);
  std::vector<int> iw(iwork_size(n), 0);
  State s;
  Work w = make_work(dw.data(), iw.data(), n, m);
  Options opt{m, factr, pgtol, maxiter, maxfun, maxls};
  lbfgsb_init(s, w, n, m, x0, l, u, nbd);
  int rounds = 0;
  auto eval = [&](State &st, const Work &wk) {
    double f;
    fg(n, wk.x, &f, wk.g);
    st.f = f;
    ++rounds;
  };
  auto eval2 = [&](State &st, double a, double b, double &ga, double &gb, double, double, double, double) {
    double xx[2] = {a, b}, gg[2], f;
    fg(2, xx, &f, gg);
    st.f = f;
    ga = gg[0];
    gb = gg[1];
    ++rounds;
  };
  if (form == 0) {
    while (lbfgsb_advance(s, w, l, u, nbd, opt) == LB_NEED_FG) {
      eval(s, w);
      if (rounds > 10000000) break;
    }
  } else if (form == 1) {
    lbfgsb_advance<true>(s, w, l, u, nbd, opt, Coop{0, 1}, eval);
  } else {
    lbfgsb_advance<true>(s, w, l, u, nbd, opt, Coop{0, 1}, eval, eval2);
  }
  for (int i = 0; i < n; ++i) {
    x_out[i] = w.x[i];
    g_out[i] = w.g[i];
  }
  *f_out = s.f;
  out_i[0] = s.nit;
  out_i[1] = s.nfev;
  out_i[2] = s.status;
  out_i[3] = s.task;
  out_i[4] = s.msg;
  return rounds;
}

// The workspace layout of make_work for (n, m): the offset in doubles of every pointer it sets, relative to dw -- snd
// and wn relative to `big` when big_outside -- in the order ws wy sy ss wt snd wn z r d t xp x g xlast glast wa rwt rwn
// rsy rsq (21), the three int arrays' offsets relative to iw (3), and sizes = {dwork_size, big_size, iwork_size}.
void lbfgsb_host_layout(int n, int m, int big_outside, int *offsets, int *int_offsets, int *sizes) {
  using namespace lbfgsb;
  std::vector<double> dw(dwork_size(n, m, big_outside != 0)), big(big_size(m));
  std::vector<int> iw(iwork_size(n));
  const Work w = make_work(dw.data(), iw.data(), n, m, big_outside ? big.data() : nullptr);
  const double *mat = big_outside ? big.data() : dw.data();
  const double *const ptrs[21] = {w.ws, w.wy, w.sy, w.ss, w.wt, nullptr, nullptr, w.z, w.r, w.d, w.t, w.xp, w.x, w.g,
                                  w.xlast, w.glast, w.wa, w.rwt, w.rwn, w.rsy, w.rsq};
  for (int i = 0; i < 21; ++i) offsets[i] = ptrs[i] ? (int)(ptrs[i] - dw.data()) : 0;
  offsets[5] = (int)(w.snd - mat);
  offsets[6] = (int)(w.wn - mat);
  int_offsets[0] = (int)(w.index - iw.data());
  int_offsets[1] = (int)(w.iwhere - iw.data());
  int_offsets[2] = (int)(w.indx2 - iw.data());
  sizes[0] = dwork_size(n, m, big_outside != 0);
  sizes[1] = big_size(m);
  sizes[2] = iwork_size(n);
}

// Returns the number of state-machine round trips.  out_i = {nit, nfev, status, task, msg}.
int lbfgsb_host_minimize(int n, int m, const double *x0, const double *l, const double *u,
                         const int *nbd, double factr, double pgtol, int maxiter, int maxfun,
                         int maxls, fg_callback fg, double *x_out, double *f_out, double *g_out,
                         int *out_i) {
  using namespace lbfgsb;
  std::vector<double> dw(dwork_size(n, m), 0.0);
  std::vector<int> iw(iwork_size(n), 0);
  State s;
  Work w = make_work(dw.data(), iw.data(), n, m);
  Options opt{m, factr, pgtol, maxiter, maxfun, maxls};
  lbfgsb_init(s, w, n, m, x0, l, u, nbd);
  int rounds = 0;
  while (lbfgsb_advance(s, w, l, u, nbd, opt) == LB_NEED_FG) {
    double f;
    fg(n, w.x, &f, w.g);
    s.f = f;
    ++rounds;
    if (rounds > 10000000) break;
  }
  for (int i = 0; i < n; ++i) {
    x_out[i] = w.x[i];
    g_out[i] = w.g[i];
  }
  *f_out = s.f;
  out_i[0] = s.nit;
  out_i[1] = s.nfev;
  out_i[2] = s.status;
  out_i[3] = s.task;
  out_i[4] = s.msg;
  return rounds;
}

// lbfgsb_host_minimize_form that also returns how often each event of lbfgsb.h occurred: out_events[EV_COUNT], in
// the order of its enum (lbfgsb_host_event_count tells EV_COUNT).
int lbfgsb_host_event_count() { return lbfgsb::EV_COUNT; }

int lbfgsb_host_minimize_events(int form, int n, int m, const double *x0, const double *l, const double *u,
                                const int *nbd, double factr, double pgtol, int maxiter, int maxfun,
                                int maxls, fg_callback fg, double *x_out, double *f_out, double *g_out,
                                int *out_i, int *out_events) {
  for (int i = 0; i < lbfgsb::EV_COUNT; ++i) lbfgsb_host_events[i] = 0;
  const int rounds = lbfgsb_host_minimize_form(form, n, m, x0, l, u, nbd, factr, pgtol, maxiter, maxfun, maxls, fg,
                                               x_out, f_out, g_out, out_i);
  for (int i = 0; i < lbfgsb::EV_COUNT; ++i) out_events[i] = lbfgsb_host_events[i];
  return rounds;
}
}
