// fit_plan_dump.hip -- what the host side of bore_mlp_fit plans, as text: return code, refusal, kernel flavour, LDS
// size and every field of the carve, for a fixed grid of requests.  A stand-alone program that includes the library as
// one translation unit (the planning functions are static); it runs on the CPU, dereferences no data pointer and
// launches nothing.  Two builds of it -- one per tree -- must print the same text when only host code changed (the
// two adapters below are the only lines that name that tree's functions).
//
//   hipcc -O1 --offload-arch=gfx950 -std=c++17 -ffp-contract=off -Wno-pass-failed -DBORE_SHAPE_MASK=0x1a \
//         -I include -I bore_amd/csrc tests/native/fit_plan_dump.hip -o fit_plan_dump && ./fit_plan_dump > plans.txt
//
// The bfloat16 fit has no plan apart from its launch, so its launches are caught instead: for its argument struct an
// overload of launch_lds stands in front of the library's and records what would have been launched.
// (BORE_SHAPE_MASK: a quick build that keeps the two wide flavours the bfloat16 entry dispatches on; the planning code
// does not read the mask.)
#include <cstdio>
#include <cstring>

#include "host_common.h"

struct FitBf16Args;
static int launch_lds(void (*kernel)(const FitBf16Args), dim3 grid, dim3 block, size_t lds_bytes, void *stream,
                      const FitBf16Args &a);
#include "bore_all.hip"

struct CaughtLaunch {
  const char *form;
  size_t lds_bytes;
  int o_tile, o_misc, o_perm, o_keys, total;
};
static CaughtLaunch g_caught;
static int launch_lds(void (*kernel)(const FitBf16Args), dim3, dim3, size_t lds_bytes, void *, const FitBf16Args &a) {
  const bool mfma = kernel == fit_bf16_mfma_kernel<3> || kernel == fit_bf16_mfma_kernel<4>;
  g_caught = CaughtLaunch{mfma ? "fit_bf16_mfma_kernel" : "fit_bf16_kernel", lds_bytes, a.o_tile, a.o_misc, a.o_perm,
                          a.o_keys, a.total};
  return 0;
}

static float *const kF = reinterpret_cast<float *>(0x1000);  // (dummy non-null pointers)
static const bore_adam_cfg kAdam = {1e-3f, 0.9f, 0.999f, 1e-7f};

static FitRequest request(const bore_mlp_desc *d, int64_t N, int batch_size, bool with_perm) {
  return FitRequest{d, 1, kF, kF, kF, reinterpret_cast<int64_t *>(kF), kF, kF, N, 1, batch_size,
                    with_perm ? reinterpret_cast<const int32_t *>(kF) : nullptr, 0, 0, 0, &kAdam, nullptr};
}

// ---- the two adapters -------------------------------------------------------------------------------------------------
static int plan_f32(const bore_mlp_desc *d, int64_t N, int batch_size, bool with_perm, FitArgs &a, size_t &lds_floats,
                    int &flavour) {
  FitPlan p{};
  const int rc = fit_build(request(d, N, batch_size, with_perm), p);
  a = p.a; lds_floats = p.lds_floats; flavour = p.flavour;
  return rc;
}
static int launch_bf16(const bore_mlp_desc *d, int64_t N, bool with_perm) {
  return fit_bf16_impl(request(d, N, BORE_BATCH_MAX, with_perm), nullptr);
}
// ---------------------------------------------------------------------------------------------------------------------

static bore_mlp_desc net(int D, std::initializer_list<int> units, int hidden_act, int out_act, int compute) {
  bore_mlp_desc d{};
  d.input_dim = D;
  d.n_layers = (int)units.size();
  int i = 0;
  for (int u : units) {
    d.units[i] = u;
    d.act[i] = i + 1 == d.n_layers ? out_act : hidden_act;
    ++i;
  }
  d.compute = compute;
  return d;
}

struct Named {
  const char *name;
  bore_mlp_desc d;
};

static void dump_f32(const Named &n, int64_t N, int B, bool with_perm, bool batch) {
  bore_batch bb{};
  bb.ids = bb.its = reinterpret_cast<const int32_t *>(kF);
  bb.n_init = 5;
  bb.cap = N;
  bore_set_batch(batch ? &bb : nullptr);
  g_bore_err[0] = 0;
  FitArgs a{};
  size_t lds_floats = 0;
  int flavour = 0;
  const int rc = plan_f32(&n.d, N, B, with_perm, a, lds_floats, flavour);
  bore_set_batch(nullptr);
  printf("%s N=%lld B=%d perm=%d batch=%d -> rc=%d", n.name, (long long)N, B, (int)with_perm, (int)batch, rc);
  if (rc) {
    printf(" \"%s\"\n", g_bore_err);
    return;
  }
  printf(" flavour=%d lds_floats=%zu | tile=%d zt=%d misc=%d stage=%d m=%d v=%d perm=%d perm2=%d keys=%d X=%d z=%d g=%d "
         "layout=%d total=%d | perm_in_lds=%d state_in_lds=%d data_in_lds=%d perm_ahead=%d | n_init=%d cap=%lld "
         "P_lds=%d tile_floats=%d\n",
         flavour, lds_floats, a.o_tile, a.o_zt, a.o_misc, a.o_stage, a.o_m, a.o_v, a.o_perm, a.o_perm2, a.o_keys, a.o_X,
         a.o_z, a.o_g, a.o_layout, a.total, a.perm_in_lds, a.state_in_lds, a.data_in_lds, a.perm_ahead, a.n_init,
         (long long)a.cap, a.L.P_lds, a.L.tile_floats);
}

// One line of the bfloat16 entry; returns a key of (rc, kernel) so that the caller finds where the form switches.
static int dump_bf16(const Named &n, int64_t N, bool with_perm, bool print) {
  g_bore_err[0] = 0;
  g_caught = CaughtLaunch{"", 0, 0, 0, 0, 0, 0};
  const int rc = launch_bf16(&n.d, N, with_perm);
  if (print) {
    printf("%s bf16 N=%lld perm=%d -> rc=%d", n.name, (long long)N, (int)with_perm, rc);
    if (rc) printf(" \"%s\"\n", g_bore_err);
    else
      printf(" %s lds_bytes=%zu | tile=%d misc=%d perm=%d keys=%d total=%d\n", g_caught.form, g_caught.lds_bytes,
             g_caught.o_tile, g_caught.o_misc, g_caught.o_perm, g_caught.o_keys, g_caught.total);
  }
  return rc ? rc : (int)strlen(g_caught.form);
}

int main() {
  const int R = BORE_ACT_RELU, S = BORE_ACT_SIGMOID, E = BORE_ACT_ELU, LIN = BORE_ACT_LINEAR, F = BORE_COMPUTE_F32;
  const Named nets[] = {
      // every static and fit-only shape (32->128-128-1 in float32: the `rounds` branch)
      {"2-16-16-1", net(2, {16, 16, 1}, R, S, F)},
      {"6-32-32-1", net(6, {32, 32, 1}, R, S, F)},
      {"16-64-64-64-1", net(16, {64, 64, 64, 1}, R, S, F)},
      {"32-128-128-1", net(32, {128, 128, 1}, R, S, F)},
      {"16-32-32-32-1", net(16, {32, 32, 32, 1}, E, LIN, F)},
      {"16-32-32-1", net(16, {32, 32, 1}, R, S, F)},
      {"16-16-16-1", net(16, {16, 16, 1}, E, S, F)},
      // the same widths on fewer inputs
      {"1-16-16-1", net(1, {16, 16, 1}, R, S, F)},
      {"4-32-32-1", net(4, {32, 32, 1}, R, S, F)},
      {"8-64-64-64-1", net(8, {64, 64, 64, 1}, R, S, F)},
      {"16-128-128-1", net(16, {128, 128, 1}, R, S, F)},
      {"4-32-32-32-1", net(4, {32, 32, 32, 1}, E, LIN, F)},
      {"8-16-16-1", net(8, {16, 16, 1}, E, S, F)},
      // run-time layouts: two that fit the LDS, one that does not, five layers
      {"5-24-12-1", net(5, {24, 12, 1}, R, S, F)},
      {"10-48-1", net(10, {48, 1}, R, LIN, F)},
      {"8-256-256-1", net(8, {256, 256, 1}, R, S, F)},
      {"8-32-32-32-32-1", net(8, {32, 32, 32, 32, 1}, R, S, F)},
      // requests the remainder of fit_build refuses: two output units, a relu output
      {"2-16-16-2", net(2, {16, 16, 2}, R, S, F)},
      {"2-16-16-1relu", net(2, {16, 16, 1}, R, R, F)},
  };
  const int64_t Ns[] = {1, 64, 100, 128, 129, 512, 513, 4000, 40000};
  for (const Named &n : nets)
    for (int64_t N : Ns)
      for (int B : {16, 64, 128})
        for (int with_perm = 0; with_perm < 2; ++with_perm)
          for (int batch = 0; batch < 2; ++batch) dump_f32(n, N, B, with_perm != 0, batch != 0);

  // the bfloat16 entry: both wide shapes, the rows around every N at which the answer changes (the form switches
  // where the shuffle outgrows the LDS beside the weight images; further on the fp32-MFMA form is refused too)
  const Named wide[] = {{"16-64-64-64-1", net(16, {64, 64, 64, 1}, R, S, BORE_COMPUTE_BF16)},
                        {"32-128-128-1", net(32, {128, 128, 1}, R, S, BORE_COMPUTE_BF16)}};
  for (const Named &n : wide)
    for (int with_perm = 0; with_perm < 2; ++with_perm) {
      int last = dump_bf16(n, 1, with_perm != 0, true);
      for (int64_t N = 2; N <= 60000; ++N) {
        const int now = dump_bf16(n, N, with_perm != 0, false);
        if (now != last) {
          dump_bf16(n, N - 1, with_perm != 0, true);
          dump_bf16(n, N, with_perm != 0, true);
        }
        last = now;
      }
      dump_bf16(n, 60000, with_perm != 0, true);
    }

  // the eight-wave choice of a launch whose plan admits it (the compute-unit count is a parameter)
  for (int n_models : {1, 256, 257})
    for (int forced : {-1, 0, 1})
      printf("w8 n_models=%d forced=%d cus=256 -> %d\n", n_models, forced, (int)fit_wants_w8(n_models, forced, 256));
  return 0;
}
