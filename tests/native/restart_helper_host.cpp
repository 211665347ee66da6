// Host check of the job board's rule (bore_amd/csrc/lbfgsb.h, JOB BOARD; the device's board is bore_argmax.hip's
// RestartJobs).  A board that does, serially and on the host, what the rule allows a helper wave to do:
//   speculate -- copies the whole workspace and runs formk with the GUESSED sets on the copy, at the top of the
//                iteration, before cauchy, freev and cmprlb have run;
//   post      -- notes whether the guess holds for the arguments formk is really called with;
//   collect   -- runs formk in its usual place, and, where the guess held, compares what it left in the wn / snd block
//                and in rwn, and its return code, with the copy's: they must be the same bytes.
// Counts come back to the caller; the optimiser's own results must be those of a run without a board.
// Two ways in: restart_helper_host_run (a shared library for tests/test_restart_helper_host.py, f and g from a Python
// callback) and, with -DRESTART_HELPER_MAIN, a program of its own over analytic objectives (built and run with
// -fsanitize=address,undefined by the same test).  Test scaffolding only.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../bore_amd/csrc/lbfgsb.h"

namespace {

enum {
  C_FORMK = 0,       // iterations that called formk (wrk set)
  C_SETS_KEPT,       // ... with nenter == 0 && ileave == n + 1
  C_SPECULATED,      // speculative runs started (the previous iteration ended with a BFGS update)
  C_GUESS_HELD,      // ... whose guess held when formk's arguments were known
  C_SAME_BYTES,      // ... and whose copy equals the live workspace byte for byte (must be all of them)
  C_MISMATCH,        // ... or not (must be 0)
  C_MOVED,           // formk calls with a variable entering or leaving
  C_MOVED_ACCEPTED,  // ... that the rule accepted (must be 0)
  C_DROPPED,         // speculative runs the iteration had no use for (cauchy failed, no free variable, wrong guess)
  C_NFREE_CHANGED,   // wrong guesses with nothing entering or leaving (nfree differs: cannot happen)
  C_COUNT
};

struct HostBoard {
  int n, m;
  long long *c;
  double *dw;  // the live workspace (make_work's dw) and its size
  int *iw;
  size_t dw_size, iw_size;
  std::vector<double> dwc;
  std::vector<int> iwc;
  bool pending = false, held = false;
  lbfgsb::IterArgs guess{};
  int guess_rc = 0;

  void speculate(const lbfgsb::IterArgs &g, const lbfgsb::Work &) {
    dwc.assign(dw, dw + dw_size);
    iwc.assign(iw, iw + iw_size);
    const lbfgsb::Work wc = lbfgsb::make_work(dwc.data(), iwc.data(), n, m);
    guess = g;
    guess_rc = lbfgsb::formk(g, wc);
    pending = true;
    ++c[C_SPECULATED];
  }
  void drop() {
    if (pending) ++c[C_DROPPED];
    pending = false;
  }
  void post(const lbfgsb::IterArgs &ia, const lbfgsb::Work &) {
    ++c[C_FORMK];
    const bool moved = ia.nenter > 0 || ia.ileave < n + 1;
    if (moved) ++c[C_MOVED];
    else ++c[C_SETS_KEPT];
    held = pending && ia.nenter == 0 && ia.ileave == ia.n + 1 && ia.nfree == guess.nfree;
    if (held && moved) ++c[C_MOVED_ACCEPTED];
    if (pending && !held) {
      if (!moved) ++c[C_NFREE_CHANGED];
      drop();
    }
  }
  int collect(const lbfgsb::IterArgs &ia, const lbfgsb::Work &w) {
    const int rc = lbfgsb::formk(ia, w);
    if (pending && held) {
      ++c[C_GUESS_HELD];
      const lbfgsb::Work wc = lbfgsb::make_work(dwc.data(), iwc.data(), n, m);
      const bool same = rc == guess_rc &&
                        std::memcmp(w.snd, wc.snd, sizeof(double) * lbfgsb::big_size(m)) == 0 &&
                        std::memcmp(w.rwn, wc.rwn, sizeof(double) * 2 * m) == 0 &&
                        ia.col == guess.col && ia.head == guess.head && ia.updatd == guess.updatd &&
                        ia.iupdat == guess.iupdat && std::memcmp(&ia.theta, &guess.theta, sizeof(double)) == 0;
      ++c[same ? C_SAME_BYTES : C_MISMATCH];
    }
    pending = false;
    return rc;
  }
};

struct Result {
  std::vector<double> x, g;
  double f;
  int info[5];
};

template <class FG>
Result run(int n, int m, const double *x0, const double *l, const double *u, const int *nbd, const lbfgsb::Options &opt,
           FG fg, long long *counts) {
  using namespace lbfgsb;
  std::vector<double> dw(dwork_size(n, m), 0.0);
  std::vector<int> iw(iwork_size(n), 0);
  State s;
  Work w = make_work(dw.data(), iw.data(), n, m);
  lbfgsb_init(s, w, n, m, x0, l, u, nbd);
  auto eval = [&](State &st, const Work &wk) {
    double f;
    fg(n, wk.x, &f, wk.g);
    st.f = f;
  };
  if (counts) {
    HostBoard board{n, m, counts, dw.data(), iw.data(), dw.size(), iw.size(), {}, {}};
    lbfgsb_advance<true>(s, w, l, u, nbd, opt, Coop{0, 1}, eval, NoTwoVariableForm{}, board);
  } else {
    lbfgsb_advance<true>(s, w, l, u, nbd, opt, Coop{0, 1}, eval);
  }
  Result r;
  r.x.assign(w.x, w.x + n);
  r.g.assign(w.g, w.g + n);
  r.f = s.f;
  r.info[0] = s.nit; r.info[1] = s.nfev; r.info[2] = s.status; r.info[3] = s.task; r.info[4] = s.msg;
  return r;
}

bool same_result(const Result &a, const Result &b) {
  return a.x.size() == b.x.size() && std::memcmp(a.x.data(), b.x.data(), 8 * a.x.size()) == 0 &&
         std::memcmp(a.g.data(), b.g.data(), 8 * a.g.size()) == 0 && std::memcmp(&a.f, &b.f, 8) == 0 &&
         std::memcmp(a.info, b.info, sizeof(a.info)) == 0;
}

}  // namespace

extern "C" {

typedef void (*fg_callback)(int n, const double *x, double *f, double *g);

int restart_helper_host_count() { return C_COUNT; }

// One problem with the board and once more without: counts[C_COUNT] are ADDED to; returns 0 when the two runs gave the
// same bits (x, f, g, nit, nfev, status, task, msg), 1 otherwise.  out_i = {nit, nfev, status, task, msg}.
int restart_helper_host_run(int n, int m, const double *x0, const double *l, const double *u, const int *nbd,
                            double factr, double pgtol, int maxiter, int maxfun, int maxls, fg_callback fg,
                            long long *counts, int *out_i) {
  const lbfgsb::Options opt{m, factr, pgtol, maxiter, maxfun, maxls};
  const Result a = run(n, m, x0, l, u, nbd, opt, fg, counts);
  const Result b = run(n, m, x0, l, u, nbd, opt, fg, nullptr);
  for (int i = 0; i < 5; ++i) out_i[i] = a.info[i];
  return same_result(a, b) ? 0 : 1;
}
}

#ifdef RESTART_HELPER_MAIN
// Analytic objectives over boxes whose optima lie inside, on faces and in corners, n = 2..7, maxcor 3 (the history
// wraps: formk's shift) and 10.
namespace {
int g_kind = 0;
void objective(int n, const double *x, double *f, double *g) {
  double v = 0.0;
  if (g_kind == 0) {  // Rosenbrock
    for (int i = 0; i < n; ++i) g[i] = 0.0;
    for (int i = 0; i + 1 < n; ++i) {
      const double a = x[i + 1] - x[i] * x[i], b = 1.0 - x[i];
      v += 100.0 * a * a + b * b;
      g[i] += -400.0 * a * x[i] - 2.0 * b;
      g[i + 1] += 200.0 * a;
    }
  } else if (g_kind == 1) {  // a tilted bowl whose minimiser lies outside the unit box: faces and corners
    for (int i = 0; i < n; ++i) {
      const double c = (i % 3 == 0) ? 1.4 : (i % 3 == 1 ? -0.3 : 0.6), d = x[i] - c;
      v += (1.0 + i) * d * d;
      g[i] = 2.0 * (1.0 + i) * d;
    }
    for (int i = 0; i + 1 < n; ++i) {
      v += 0.3 * x[i] * x[i + 1];
      g[i] += 0.3 * x[i + 1];
      g[i + 1] += 0.3 * x[i];
    }
  } else {  // y = sum x (the corner) plus a ripple that keeps the line searches busy
    for (int i = 0; i < n; ++i) {
      v += x[i] + 0.05 * std::sin(9.0 * x[i]);
      g[i] = 1.0 + 0.45 * std::cos(9.0 * x[i]);
    }
  }
  *f = v;
}
}  // namespace

int main() {
  long long counts[C_COUNT] = {0};
  int problems = 0, different = 0;
  unsigned long long rng = 0x9e3779b97f4a7c15ull;
  auto uniform = [&]() {
    rng = rng * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(rng >> 11) / 9007199254740992.0;
  };
  for (g_kind = 0; g_kind < 3; ++g_kind)
    for (int n = 2; n <= 7; ++n)
      for (int m : {3, 10})
        for (int pattern = 0; pattern < 3; ++pattern)
          for (int start = 0; start < 4; ++start) {
            std::vector<double> x0(n), l(n), u(n);
            std::vector<int> nbd(n);
            for (int i = 0; i < n; ++i) {
              x0[i] = -0.1 + 1.2 * uniform();
              l[i] = 0.0;
              u[i] = 1.0;
              nbd[i] = pattern == 0 ? 2 : (pattern == 1 ? (i % 2 ? 3 : 1) : i % 4);
              if (g_kind == 2 && nbd[i] != 2 && nbd[i] != 1) nbd[i] = 2;  // (unbounded below: the sum runs off)
            }
            int info[5];
            different += restart_helper_host_run(n, m, x0.data(), l.data(), u.data(), nbd.data(), 1e7, 1e-8, 60, 2000, 20,
                                                 objective, counts, info);
            ++problems;
          }
  std::printf("problems %d different %d formk %lld sets_kept %lld speculated %lld guess_held %lld same_bytes %lld "
              "mismatch %lld moved %lld moved_accepted %lld dropped %lld nfree_changed %lld\n",
              problems, different, counts[C_FORMK], counts[C_SETS_KEPT], counts[C_SPECULATED], counts[C_GUESS_HELD],
              counts[C_SAME_BYTES], counts[C_MISMATCH], counts[C_MOVED], counts[C_MOVED_ACCEPTED], counts[C_DROPPED],
              counts[C_NFREE_CHANGED]);
  const bool ok = different == 0 && counts[C_MISMATCH] == 0 && counts[C_MOVED_ACCEPTED] == 0 &&
                  counts[C_SAME_BYTES] == counts[C_GUESS_HELD] && counts[C_GUESS_HELD] > 0 && counts[C_MOVED] > 0;
  std::printf(ok ? "restart helper rule ok\n" : "restart helper rule FAILED\n");
  return ok ? 0 : 1;
}
#endif
