// acq_plan_dump.hip -- what the host side of the acquisition entry points (bore_lbfgsb_minimize, bore_screen_topk,
// bore_sample_screen_topk) would launch, as text: return code, refusal, kernel, grid, block, LDS size and every field
// of the carve, for a fixed grid of requests.  A stand-alone program that includes the library as one translation unit;
// it dereferences no data pointer and launches nothing: every kernel launch of the library is caught and recorded
// (hipLaunchKernelGGL and the calls around it are redirected below), so the entry points themselves are called and
// two builds of this file -- one per tree -- must print the same text when only host code changed.  The lines that
// begin with "plan " ask this tree's pointer-free plans directly (the kernel enum, the pool, the split); a tree
// without lbfgsb_plan / screen_plan builds the file with -DACQ_DUMP_NO_PLANS and prints none of them.
//
//   hipcc -O1 --offload-arch=gfx950 -std=c++17 -ffp-contract=off -Wno-pass-failed -I include -I bore_amd/csrc \
//         tests/native/acq_plan_dump.hip -o acq_plan_dump && ./acq_plan_dump > plans.txt
//
// Without an argument: the whole grid, on the CPU -- no HIP call is made at all (the device query answers "no device",
// so the library counts 256 compute units, the MI355X's number).  The requests whose optimiser matrices go to the device
// pool (32->128-128-1 in bfloat16 on eight waves) need an allocation: with the argument `pooled` the program prints
// that section alone with the real device behind big_pool -- still without a launch -- and `pooled0` prints it with
// BORE_LBFGSB_BIG=0 (no pool: runs anywhere).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

struct LbfgsbArgs;
struct ScreenArgs;
template <class K, class... T>
static void caught_launch(K, dim3, dim3, size_t, hipStream_t, const T &...) {}  // (any other kernel: not launched either)
static void caught_launch(void (*kernel)(const LbfgsbArgs), dim3 grid, dim3 block, size_t lds, hipStream_t,
                          const LbfgsbArgs &a);
static void caught_launch(void (*kernel)(const ScreenArgs), dim3 grid, dim3 block, size_t lds, hipStream_t,
                          const ScreenArgs &a);
static bool g_real_device = false;
static hipError_t dump_get_device(int *dev) { return g_real_device ? (hipGetDevice)(dev) : hipErrorNoDevice; }
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernel, grid, block, lds, stream, ...) caught_launch(kernel, grid, block, lds, stream, __VA_ARGS__)
#define hipGetLastError() hipSuccess
#define hipGetDevice(dev) dump_get_device(dev)

#include "host_common.h"
// (in front of the library's allow_lds for every kernel that takes one argument struct: its refusal, no HIP call)
template <class A>
static int allow_lds(void (*)(const A), size_t bytes) {
  if (bytes > BORE_LDS_BYTES)
    return fail(BORE_E_UNSUPPORTED, "model needs %zu B of LDS per workgroup (> %d); %s", bytes, BORE_LDS_BYTES,
                kStreamedElsewhere);
  return 0;
}
#include "bore_all.hip"

// ---- the caught launches ------------------------------------------------------------------------------------------
struct Caught {
  char kernel[48];
  dim3 grid, block;
  size_t lds;
};
static Caught g_caught[2];
static int g_n_caught;
static LbfgsbArgs g_lb;
static ScreenArgs g_sc;

template <int... S, class F>
static void each_flavour(FlavourList<S...>, F f) { (f(std::integral_constant<int, S>{}), ...); }
// names the kernel among the instantiations the library's launches name (and no others)
#define NAME_IF(LIST, KERNEL, LABEL)                                          \
  each_flavour(LIST{}, [&](auto S) {                                          \
    if constexpr (bore_flavour_on(S()))                                       \
      if (k == (KERNEL)) snprintf(c.kernel, sizeof(c.kernel), LABEL, (int)S()); \
  })
static Caught &caught(dim3 grid, dim3 block, size_t lds) {
  Caught &c = g_caught[g_n_caught < 2 ? g_n_caught : 1];
  ++g_n_caught;
  snprintf(c.kernel, sizeof(c.kernel), "?");
  c.grid = grid; c.block = block; c.lds = lds;
  return c;
}
static void caught_launch(void (*k)(const LbfgsbArgs), dim3 grid, dim3 block, size_t lds, hipStream_t, const LbfgsbArgs &a) {
  Caught &c = caught(grid, block, lds);
  g_lb = a;
  NAME_IF(AcqFlavours, (lbfgsb_kernel<S(), false>), "lbfgsb_kernel<%d,f32>");
  NAME_IF(WideFlavours, (lbfgsb_kernel<S(), true>), "lbfgsb_kernel<%d,bf16>");
  NAME_IF(NarrowWavesFlavours, (lbfgsb_kernel_occ2<S()>), "lbfgsb_kernel_occ2<%d>");
  NAME_IF(NarrowWavesFlavours, (lbfgsb_kernel_w12<S(), false>), "lbfgsb_kernel_w12<%d>");
  NAME_IF(FlavourList<3>, (lbfgsb_kernel_w8<S(), false>), "lbfgsb_kernel_w8<%d,f32>");
  NAME_IF(WideFlavours, (lbfgsb_kernel_w8<S(), true>), "lbfgsb_kernel_w8<%d,bf16>");
}
static void caught_launch(void (*k)(const ScreenArgs), dim3 grid, dim3 block, size_t lds, hipStream_t, const ScreenArgs &a) {
  Caught &c = caught(grid, block, lds);
  g_sc = a;
  NAME_IF(AcqFlavours, (screen_topk_kernel<S(), false, 0>), "screen<%d,f32,0>");
  NAME_IF(WideFlavours, (screen_topk_kernel<S(), true, 0>), "screen<%d,bf16,0>");
  NAME_IF(WideFlavours, (screen_topk_kernel<S(), false, 1>), "screen<%d,f32,1>");
  NAME_IF(WideFlavours, (screen_topk_kernel<S(), false, 2>), "screen<%d,f32,2>");
  NAME_IF(WideFlavours, (screen_topk_kernel<S(), true, 1>), "screen<%d,bf16,1>");
  NAME_IF(WideFlavours, (screen_topk_kernel<S(), true, 2>), "screen<%d,bf16,2>");
}

// ---- requests -------------------------------------------------------------------------------------------------------
static float *const kF = reinterpret_cast<float *>(0x1000);  // (dummy non-null pointers)
static double *const kD = reinterpret_cast<double *>(0x1000);
static int32_t *const kI = reinterpret_cast<int32_t *>(0x1000);
static double g_lo[BORE_DIM_MAX], g_hi[BORE_DIM_MAX];  // (the box is read: [0, 1]^D)

static bore_mlp_desc net(int D, std::initializer_list<int> units, int hidden_act, int out_act) {
  bore_mlp_desc d{};
  d.input_dim = D;
  d.n_layers = (int)units.size();
  int i = 0;
  for (int u : units) {
    d.units[i] = u;
    d.act[i] = i + 1 == d.n_layers ? out_act : hidden_act;
    ++i;
  }
  return d;
}
struct Named {
  const char *name;
  bore_mlp_desc d;
};
struct Knob {
  const char *name, *value;
};
static const char *const kKnobs[] = {"BORE_LBFGSB_COOP_GRID", "BORE_LBFGSB_WAVES", "BORE_LBFGSB_BIG",
                                     "BORE_LBFGSB_QUEUE",     "BORE_LBFGSB_OCC2",  "BORE_SCREEN_SPLIT"};
static void set_knobs(std::initializer_list<Knob> knobs) {
  for (const char *k : kKnobs) unsetenv(k);
  for (const Knob &k : knobs) setenv(k.name, k.value, 1);
}
static void print_knobs() {
  for (const char *k : kKnobs)
    if (getenv(k)) printf(" %s=%s", k + 5, getenv(k));
}
static void set_batch(bool on, int n_init) {
  bore_batch bb{};
  bb.ids = bb.its = kI;
  bb.result = kD;
  bb.flag = kI;
  bb.n_init = n_init;
  bb.cap = 64;
  bore_set_batch(on ? &bb : nullptr);
}

static void dump_restarts(const Named &n, int compute, int n_models, int R, int maxcor, bool batch) {
  bore_mlp_desc d = n.d;
  d.compute = compute;
  const bore_lbfgsb_opts opts = {maxcor, 15000, 15000, 20, 2.22e-9, 1e-5};
  set_batch(batch, 5);
  g_bore_err[0] = 0;
  g_n_caught = 0;
  const int rc = bore_lbfgsb_minimize(&d, n_models, kF, BORE_T_SIGMOID, 1, kD, R, g_lo, g_hi, &opts, kD, kD, kD, kI, nullptr);
  printf("L %s %s models=%d R=%d m=%d batch=%d", n.name, compute == BORE_COMPUTE_BF16 ? "bf16" : "f32", n_models, R,
         maxcor, (int)batch);
  print_knobs();
  printf(" -> rc=%d", rc);
  if (rc) printf(" \"%s\"\n", g_bore_err);
  else {
    const LbfgsbArgs &a = g_lb;
    const Caught &c = g_caught[0];
    printf(" launches=%d %s blocks=%u grid.x=%u waves=%u lds_floats=%zu | tile=%d vals=%d box=%d prob=%d prob_floats=%d "
           "state=%d dw=%d iw=%d res=%d queue=%d layout=%d total=%d | PB=%d queue=%d big=%d R=%d max_rounds=%d d_in=%d "
           "sign=%g by_store=%d ids=%d n_init=%d cap=%lld | P_lds=%d tile_floats=%d\n",
           g_n_caught, c.kernel, c.grid.y, c.grid.x, c.block.x / 64, c.lds / 4, a.o_tile, a.o_vals, a.o_box, a.o_prob,
           a.prob_floats, a.o_state, a.o_dw, a.o_iw, a.o_res, a.o_queue, a.o_layout, a.total, a.PB, a.queue,
           (int)(a.big_wave != 0) + 2 * (int)(a.big != nullptr), a.R, a.max_rounds, a.d_in, (double)a.sign,
           a.flag_by_store, (int)(a.ids != nullptr), a.n_init, a.cap, a.L.P_lds, a.L.tile_floats);
  }
#ifndef ACQ_DUMP_NO_PLANS
  if (d.input_dim >= 1 && d.input_dim <= BORE_DIM_MAX) {  // (what lbfgsb_check_args sees to before the plan is asked)
    LbfgsbPlan p;
    g_bore_err[0] = 0;
    const int prc = lbfgsb_plan(&d, n_models, R, maxcor, acq_knobs(), 256, g_batch, true, p);
    printf("plan L rc=%d", prc);
    if (prc) printf(" \"%s\"\n", g_bore_err);
    else
      printf(" kernel=%d flavour=%d slots=%d waves=%d blocks=%d lds_floats=%zu pool_doubles=%zu PB=%d queue=%d total=%d\n",
             (int)p.kernel, p.flavour, p.slots, p.waves, p.blocks, p.lds_floats, p.pool_doubles, p.a.PB, p.a.queue, p.a.total);
  }
#endif
  set_batch(false, 0);
}

static void dump_screen(const Named &n, int compute, int n_models, int64_t n_samples, int R, bool pred, bool sampled,
                        bool batch) {
  bore_mlp_desc d = n.d;
  d.compute = compute;
  set_batch(batch, 5);
  g_bore_err[0] = 0;
  g_n_caught = 0;
  float *const pr = pred ? kF : nullptr;
  const int rc = sampled ? bore_sample_screen_topk(&d, n_models, kF, 7, 3, 1, n_samples, g_lo, g_hi, R, kD, kI, pr, nullptr)
                         : bore_screen_topk(&d, n_models, kF, kD, n_samples, 0, R, kD, kI, pr, nullptr);
  printf("S %s %s models=%d Ns=%lld R=%d pred=%d sampled=%d batch=%d", n.name, compute == BORE_COMPUTE_BF16 ? "bf16" : "f32",
         n_models, (long long)n_samples, R, (int)pred, (int)sampled, (int)batch);
  print_knobs();
  printf(" -> rc=%d", rc);
  if (rc) printf(" \"%s\"\n", g_bore_err);
  else {
    const ScreenArgs &a = g_sc;
    printf(" launches=%d", g_n_caught);
    for (int i = 0; i < g_n_caught && i < 2; ++i)
      printf(" %s grid=(%u,%u) lds_floats=%zu", g_caught[i].kernel, g_caught[i].grid.x, g_caught[i].grid.y, g_caught[i].lds / 4);
    printf(" | tile=%d box=%d keys=%d layout=%d total=%d | n_pad=%d R=%d sampled=%d seed=%llu model0=%lld draw=%lld "
           "ids=%d d_in=%d | P_lds=%d tile_floats=%d\n",
           a.o_tile, a.o_box, a.o_keys, a.o_layout, a.total, a.n_pad, a.R, a.sampled, a.seed, a.model0, a.draw,
           (int)(a.ids != nullptr), a.d_in, a.L.P_lds, a.L.tile_floats);
  }
#ifndef ACQ_DUMP_NO_PLANS
  ScreenPlan p;
  g_bore_err[0] = 0;
  const int prc = screen_plan(&d, n_models, n_samples, R, pred, acq_knobs(), 256, g_batch != nullptr, p);
  printf("plan S rc=%d", prc);
  if (prc) printf(" \"%s\"\n", g_bore_err);
  else printf(" flavour=%d lds_floats=%zu parts=%d total=%d\n", p.flavour, p.lds_floats, p.parts, p.a.total);
#endif
  set_batch(false, 0);
}

static const int kStarts[] = {1, 3, 4, 5, 8, 12, 13, 16, 17, 21, 70, 1024};
static const int kModels[] = {1, 3, 64, 65, 256};
static const int kComputes[] = {BORE_COMPUTE_F32, BORE_COMPUTE_BF16};

// The requests whose plan may want the device pool, under every setting of the two knobs that decide it.
static void pooled_section(const Named &wide, bool big_off) {
  for (int maxcor : {32, 10, 4})  // (the largest slots first: one pool)
    for (int waves = 0; waves < 3; ++waves)
      for (int big = big_off ? 0 : -1; big < (big_off ? 1 : 2); ++big)
        for (const char *queue : {"", "0", "7"}) {
          set_knobs({});
          if (waves) setenv("BORE_LBFGSB_WAVES", waves == 1 ? "4" : "8", 1);
          if (big >= 0) setenv("BORE_LBFGSB_BIG", big ? "1" : "0", 1);
          if (*queue) setenv("BORE_LBFGSB_QUEUE", queue, 1);
          for (int n_models : kModels)
            for (int R : kStarts) dump_restarts(wide, BORE_COMPUTE_BF16, n_models, R, maxcor, false);
        }
  set_knobs({});
}

int main(int argc, char **argv) {
  const int R = BORE_ACT_RELU, S = BORE_ACT_SIGMOID, E = BORE_ACT_ELU, LIN = BORE_ACT_LINEAR;
  for (int d = 0; d < BORE_DIM_MAX; ++d) g_hi[d] = 1.0;
  const Named nets[] = {
      // the five acquisition static shapes, and the plugin's network on fewer inputs
      {"2-16-16-1", net(2, {16, 16, 1}, R, S)},
      {"6-32-32-1", net(6, {32, 32, 1}, R, S)},
      {"16-64-64-64-1", net(16, {64, 64, 64, 1}, R, S)},
      {"32-128-128-1", net(32, {128, 128, 1}, R, S)},
      {"16-32-32-32-1", net(16, {32, 32, 32, 1}, E, LIN)},
      {"9-32-32-32-1", net(9, {32, 32, 32, 1}, E, LIN)},
      // run-time layouts: two that fit, one whose problem state does not, and a net with two output units
      {"5-24-12-1", net(5, {24, 12, 1}, R, S)},
      {"10-48-1", net(10, {48, 1}, R, LIN)},
      {"8-176-176-1", net(8, {176, 176, 1}, R, S)},
      {"2-16-16-2", net(2, {16, 16, 2}, R, S)},
  };
  const Named &wide = nets[3];
  if (argc > 1) {
    g_real_device = !strcmp(argv[1], "pooled");
    pooled_section(wide, !g_real_device);
    return 0;
  }

  // restarts, knobs unset: the whole grid, batch mode off and on
  set_knobs({});
  for (const Named &n : nets)
    for (int compute : kComputes)
      for (int n_models : kModels)
        for (int R0 : kStarts)
          for (int maxcor : {4, 10, 32})
            for (int batch = 0; batch < 2; ++batch) dump_restarts(n, compute, n_models, R0, maxcor, batch != 0);
  // batch mode with an incomplete bore_batch (no result block), and with n_init and dedup carried over
  for (int R0 : {4, 16, 17}) {
    bore_batch bb{};
    bb.ids = bb.its = kI;
    bb.flag = kI;
    bore_set_batch(&bb);
    const bore_lbfgsb_opts opts = {10, 15000, 15000, 20, 2.22e-9, 1e-5};
    const int rc = bore_lbfgsb_minimize(&nets[0].d, 3, kF, BORE_T_SIGMOID, 1, kD, R0, g_lo, g_hi, &opts, kD, kD, kD, kI, nullptr);
    printf("L 2-16-16-1 incomplete batch R=%d -> rc=%d \"%s\"\n", R0, rc, g_bore_err);
    bore_set_batch(nullptr);
  }
  // each knob at the values the GPU tests use (tests/test_gpu_argmax.py), and their combinations there; batch mode
  // reads none of them (one setting shows it)
  const std::initializer_list<Knob> settings[] = {
      {{"BORE_LBFGSB_COOP_GRID", "4194304"}}, {{"BORE_LBFGSB_COOP_GRID", "0"}},
      {{"BORE_LBFGSB_OCC2", "0"}}, {{"BORE_LBFGSB_OCC2", "1"}},
      {{"BORE_LBFGSB_WAVES", "4"}}, {{"BORE_LBFGSB_WAVES", "8"}}, {{"BORE_LBFGSB_WAVES", "12"}},
      {{"BORE_LBFGSB_QUEUE", "0"}}, {{"BORE_LBFGSB_QUEUE", "3"}}, {{"BORE_LBFGSB_QUEUE", "7"}},
      {{"BORE_LBFGSB_QUEUE", "7"}, {"BORE_LBFGSB_WAVES", "8"}, {"BORE_LBFGSB_OCC2", "1"}},
      {{"BORE_LBFGSB_QUEUE", "7"}, {"BORE_LBFGSB_WAVES", "8"}, {"BORE_LBFGSB_BIG", "1"}},
      {{"BORE_LBFGSB_QUEUE", "0"}, {"BORE_LBFGSB_WAVES", "8"}, {"BORE_LBFGSB_BIG", "1"}},
      {{"BORE_LBFGSB_QUEUE", "7"}, {"BORE_LBFGSB_WAVES", "8"}, {"BORE_LBFGSB_BIG", "0"}},
      {{"BORE_LBFGSB_QUEUE", "7"}, {"BORE_LBFGSB_WAVES", "12"}}, {{"BORE_LBFGSB_QUEUE", "0"}, {"BORE_LBFGSB_WAVES", "12"}},
      {{"BORE_LBFGSB_QUEUE", "5"}, {"BORE_LBFGSB_WAVES", "4"}, {"BORE_LBFGSB_OCC2", "1"}},
      {{"BORE_LBFGSB_BIG", "0"}}, {{"BORE_LBFGSB_BIG", "1"}},
  };
  for (const auto &knobs : settings) {
    set_knobs(knobs);
    for (const Named &n : nets)
      for (int compute : kComputes)
        for (int n_models : kModels)
          for (int R0 : kStarts) dump_restarts(n, compute, n_models, R0, 10, false);
  }
  set_knobs({{"BORE_LBFGSB_COOP_GRID", "0"}, {"BORE_LBFGSB_WAVES", "12"}, {"BORE_LBFGSB_QUEUE", "7"}, {"BORE_LBFGSB_OCC2", "1"},
             {"BORE_LBFGSB_BIG", "1"}});
  for (const Named &n : nets)
    for (int R0 : kStarts) dump_restarts(n, BORE_COMPUTE_F32, 65, R0, 10, true);
  // the pooled requests once more, on their own and without the pool
  pooled_section(wide, true);
  // more than 65 535 workgroups per model: past the one-problem-per-wave grid by size, and within it without the queue
  dump_restarts(nets[0], BORE_COMPUTE_F32, 1, (1 << 24) + 4, 10, false);
  dump_restarts(nets[0], BORE_COMPUTE_F32, 1, 4 * 65536, 10, false);
  set_knobs({{"BORE_LBFGSB_QUEUE", "0"}});
  dump_restarts(nets[0], BORE_COMPUTE_F32, 1, 4 * 65536, 10, false);
  dump_restarts(nets[0], BORE_COMPUTE_F32, 1, 4 * 65535, 10, false);
  set_knobs({});
  // screening beyond the grid: n_samples out of range, the plain form in batch mode
  for (int64_t Ns : {0, (1 << 20) + 1}) dump_screen(nets[0], BORE_COMPUTE_F32, 1, Ns, 1, false, true, false);
  dump_screen(nets[0], BORE_COMPUTE_F32, 1, 256, 4, false, false, true);

  // screening: n_samples across a power of two and across n_blocks / 8 >= 4 (512 rows), with and without pred, both
  // forms, batch mode (which takes the sampled form only), the split knob unset / 0 / 1
  for (const char *split : {"", "0", "1"}) {
    set_knobs({});
    if (*split) setenv("BORE_SCREEN_SPLIT", split, 1);
    for (const Named &n : nets)
      for (int compute : kComputes)
        for (int n_models : kModels)
          for (int64_t Ns : {1, 16, 255, 256, 257, 496, 511, 512, 513, 1024, 1025, 8192, 100000, 1 << 20})
            for (int R0 : {1, 5, 300})
              for (int pred = 0; pred < 2; ++pred)
                for (int form = 0; form < (*split ? 2 : 3); ++form)  // (plain, sampled, sampled in batch mode)
                  dump_screen(n, compute, n_models, Ns, R0, pred != 0, form > 0, form == 2);
  }
  set_knobs({});
  return 0;
}
