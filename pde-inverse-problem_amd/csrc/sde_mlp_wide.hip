// sde_mlp_wide.hip — the learned potential V_theta = V_hypothesis at widths 21..256 (core/model.py:32-62) as a
// potential of the simulator and as a batch function (gfx950):
//   pdeinv_mlp_potential_wide      V_theta(x_r) and grad V_theta(x_r) over a batch;
//   pdeinv_sde_simulate_mlp_wide   utils/sampling_utils.py:6-52 (update_step, underdamped_langevin_dynamics_scan)
//                                  with grad U = grad V_theta: q and p of a particle in registers and its
//                                  activations in LDS across all n_steps + 1 updates, one launch.
//
// Both run mlpw::wide_grad (mlp_tile_wide.h): 16 particles per wave tile, every product a
// v_mfma_f32_16x16x4_f32, the weights streamed through LDS slices when the image does not fit. The potential entry
// point is therefore the direct test of the simulator's drift, as pdeinv_mlp_potential is of the narrow one.
//
// Simulator: sim_tile of sde_mlp_tile.h (the layout is described there) with wide_grad on the block's feed as the
// gradient. Blocks are persistent (at most one per CU) and step through block tiles of `waves` wave tiles; since
// the slice hand-over is a block barrier, every wave runs every block tile and update (without a tile of its own:
// on a clamped row, no stores).
#include <math.h>

#include "common.h"
#include "mlp_engine.h"
#include "mlp_tile.h"
#include "mlp_tile_wide.h"
#include "sde_common.h"
#include "sde_mlp_tile.h"

namespace pdeinv {
namespace mlpw {

using mlpq::potential_checks;
using mlpq::sim_checked_args;
using mlpq::sim_tile;
using mlpq::store_potential;
using mlpq::TileSimArgs;

struct WideSimArgs {
  TileSimArgs s;
  WideNet net;
};

// the LDS regions of a block: [biases | image or two slices | per wave: checkpoints, gradient slot, row slot]
struct Regions {
  const f32x4* bias4;
  f32x4* act;
  float *gslot, *zslot;
};
__device__ __forceinline__ Regions regions(const WideNet& t, f32x4* lds4, int wib) {
  const size_t w4 = t.resident ? (size_t)t.units * 64 : (size_t)2 * kSlice4;
  const size_t per_wave4 = (size_t)t.L * t.MB * 64 + (kSlotG + kSlotZ) / 4;
  f32x4* mine = lds4 + t.bias_floats / 4 + w4 + wib * per_wave4;
  Regions r;
  r.bias4 = lds4;
  r.act = mine;
  r.gslot = reinterpret_cast<float*>(mine + (size_t)t.L * t.MB * 64);
  r.zslot = r.gslot + kSlotG;
  return r;
}

__global__ __launch_bounds__(kWavesMax* kWave) void sde_mlp_wide_kernel(WideSimArgs a, const float* __restrict__ z0,
                                                                        float* __restrict__ traj,
                                                                        float* __restrict__ tau,
                                                                        float* __restrict__ last) {
  extern __shared__ f32x4 lds4[];
  Feed f;
  feed_init(f, a.net, lds4);
  const int lane = threadIdx.x & (kWave - 1);
  const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const Regions R = regions(a.net, lds4, wib);
  const int waves = a.net.waves;
  const int64_t n_btiles = (a.s.n_tiles + waves - 1) / waves;
  auto grad = [&](const float (&q)[2]) {
    float unused;
    return wide_grad<false>(a.net, f, R.bias4, R.act, lane, q, unused);
  };
  for (int64_t bt = blockIdx.x; bt < n_btiles; bt += gridDim.x)
    sim_tile<2>(a.s, a.s.noise != nullptr, a.net.D, lane, (bt * waves + wib) * 16, R.gslot, R.zslot, z0, traj, tau,
                last, grad);
}

__global__ __launch_bounds__(kWavesMax* kWave) void mlp_potential_wide_kernel(WideNet net,
                                                                              const float* __restrict__ x, int64_t n,
                                                                              int64_t ld, int64_t n_tiles,
                                                                              float* __restrict__ value,
                                                                              float* __restrict__ grad) {
  extern __shared__ f32x4 lds4[];
  Feed f;
  feed_init(f, net, lds4);
  const int lane = threadIdx.x & (kWave - 1), p = lane & 15, g = lane >> 4;
  const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const Regions R = regions(net, lds4, wib);
  const int D = net.D, waves = net.waves;
  const int64_t n_btiles = (n_tiles + waves - 1) / waves;
  for (int64_t bt = blockIdx.x; bt < n_btiles; bt += gridDim.x) {
    const int64_t i_raw = (bt * waves + wib) * 16 + p;
    const bool active = i_raw < n;
    const int64_t i = active ? i_raw : n - 1;
    float xr[2];
    lane_dims<2>(x + i * ld, D, g, xr);
    float val;
    const f32x4 ga = wide_grad<true>(net, f, R.bias4, R.act, lane, xr, val);
    store_potential(active, i, g, D, val, ga, value, grad);
  }
}

// ---- host ----------------------------------------------------------------------------------------
static bool envelope(const pdeinv_mlp_shape* s) {
  return wide_envelope(s->dim, s->n_layers, s->width, s->out_features);
}
static bool shape_ok(const pdeinv_mlp_shape* s) {
  return wide_shape_ok(s->dim, s->n_layers, s->width, s->out_features);
}
static WideNet net_of(const pdeinv_mlp_shape* s, const float* img) {
  return wide_net(s->dim, s->n_layers, s->width, s->out_features, img);
}
static size_t ws_bytes(const pdeinv_mlp_shape* s) {
  size_t total = 0;
  take(total, sizeof(float) * wide_image_floats(net_of(s, nullptr)));
  return total;
}
// persistent blocks, at most one per CU; a block steps through block tiles of `waves` wave tiles. One per CU also
// where a small resident net's LDS would admit two (e.g. 64.5 KiB for 3 -> 21 x 2 -> 7): a choice for one grid
// rule, not a measured one
static int grid_of(int64_t n_tiles, int waves) {
  const int64_t need = (n_tiles + waves - 1) / waves, cap = (int64_t)device_cus();
  return (int)(need < cap ? need : cap);
}

#define WIDE_ENVELOPE_TEXT                                                                                      \
  "dim <= 8, 21 <= width <= 256, n_layers >= 1 with 16 * ceil(width / 16) * n_layers <= 512, out_features <= 64 " \
  "(width <= 20: the narrow entry point)"

}  // namespace mlpw
}  // namespace pdeinv

using namespace pdeinv;
using namespace pdeinv::mlpw;

extern "C" int pdeinv_sde_simulate_mlp_wide_supported(const pdeinv_mlp_shape* s) {
  return s && envelope(s) ? 1 : 0;  // every net of the envelope has a plan (wide_net)
}

extern "C" size_t pdeinv_mlp_potential_wide_workspace_bytes(const pdeinv_mlp_shape* s, int64_t n) {
  if (!s || n < 0 || !pdeinv_sde_simulate_mlp_wide_supported(s)) return 0;
  return ws_bytes(s);
}

extern "C" size_t pdeinv_sde_simulate_mlp_wide_workspace_bytes(const pdeinv_sde_desc* d, const pdeinv_mlp_shape* s) {
  if (!d || !s || !pdeinv_sde_simulate_mlp_wide_supported(s)) return 0;
  return ws_bytes(s);
}

extern "C" int pdeinv_mlp_potential_wide(const pdeinv_mlp_shape* s, const float* params, const float* x, int64_t n,
                                         int64_t ld, float* value, float* grad, void* ws, void* stream) {
  int64_t ldx;
  bool run;
  int rc = potential_checks("mlp_potential_wide", s, shape_ok, envelope, "the wide tile covers " WIDE_ENVELOPE_TEXT,
                            params, x, n, ld, value, grad, ws, ldx, run);
  if (rc || !run) return rc;
  hipStream_t st = (hipStream_t)stream;
  const WideNet net = net_of(s, (const float*)ws);
  rc = wide_build_image(net, params, (float*)ws, st);
  if (rc) return rc;
  const int64_t n_tiles = (n + 15) / 16;
  const dim3 gr((unsigned)grid_of(n_tiles, net.waves)), bl((unsigned)(net.waves * kWave));
  allow_lds(mlp_potential_wide_kernel);
  hipLaunchKernelGGL(mlp_potential_wide_kernel, gr, bl, wide_lds_bytes(net), st, net, x, n, ldx, n_tiles, value,
                     grad);
  return check_launch("mlp_potential_wide_kernel");
}

extern "C" int pdeinv_sde_simulate_mlp_wide(const pdeinv_sde_desc* d, const pdeinv_mlp_shape* s, const float* params,
                                            const float* z0, float* traj, float* tau, float* last, void* ws,
                                            void* stream) {
  WideSimArgs a{};
  int rc = sim_checked_args("sde_mlp_wide", d, s, shape_ok, envelope,
                            "the wide learned-potential simulator covers " WIDE_ENVELOPE_TEXT, params, z0, traj, tau,
                            last, ws, a.s);
  if (rc || a.s.N == 0) return rc;
  hipStream_t st = (hipStream_t)stream;
  const WideNet net = net_of(s, (const float*)ws);
  rc = wide_build_image(net, params, (float*)ws, st);
  if (rc) return rc;
  a.net = net;
  const dim3 gr((unsigned)grid_of(a.s.n_tiles, net.waves)), bl((unsigned)(net.waves * kWave));
  allow_lds(sde_mlp_wide_kernel);
  hipLaunchKernelGGL(sde_mlp_wide_kernel, gr, bl, wide_lds_bytes(net), st, a, z0, traj, tau, last);
  return check_launch("sde_mlp_wide_kernel");
}
