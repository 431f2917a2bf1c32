// sde_mlp.hip — the learned potential V_theta = V_hypothesis (core/model.py:32-62: tanh layers, Dense(40), sum of
// squares) as a potential of the simulator and as a batch function (gfx950):
//   pdeinv_mlp_potential      V_theta(x_r) and grad V_theta(x_r) over a batch — what the reference's commented-out
//                             quality metric "relative error of gradient estimation initial / terminal" needs
//                             (methods/consistency_instances/kinetic_fokker_planck.py:81-91);
//   pdeinv_sde_simulate_mlp   utils/sampling_utils.py:6-52 (update_step, underdamped_langevin_dynamics_scan) with
//                             grad U = grad V_theta: every update of a particle in registers.
//
// Both run mlpq::tile_grad (mlp_tile.h): 16 rows per wave tile, every product a v_mfma_f32_16x16x4_f32, layers
// chained in registers through the P layout, the output layer folded into a 20 x 20 quadratic form. The potential
// entry point is therefore the direct test of the simulator's drift.
//
// Simulator: sim_tile of sde_mlp_tile.h (the layout is described there) with tile_grad on the block's LDS image as
// the gradient. Blocks are persistent and their waves stride over the tiles.
#include <math.h>

#include "common.h"
#include "mlp_engine.h"
#include "mlp_tile.h"
#include "sde_common.h"
#include "sde_mlp_tile.h"

namespace pdeinv {
namespace mlps {

using namespace mlpq;

constexpr int kWavesB = 8;                 // waves per block: two blocks per CU = 4 waves per SIMD
constexpr int kThreads = kWavesB * kWave;
constexpr int kSlot = kSlotG + kSlotZ;     // floats per wave

struct SimArgs {
  TileSimArgs s;
  TileNet net;
};

template <int KD, bool EXPLICIT>
__global__ __launch_bounds__(kThreads) void sde_mlp_kernel(SimArgs a, const float* __restrict__ z0,
                                                           float* __restrict__ traj, float* __restrict__ tau,
                                                           float* __restrict__ last) {
  extern __shared__ f32x4 lds4[];
  float* img = reinterpret_cast<float*>(lds4);
  stage_image(lds4, a.net);
  __syncthreads();
  const int lane0 = threadIdx.x & (kWave - 1);
  const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  float* gslot = img + a.net.img_floats + wib * kSlot;
  const int64_t wave = (int64_t)blockIdx.x * kWavesB + wib;
  const int64_t n_waves = (int64_t)gridDim.x * kWavesB;
  auto grad = [&](const float (&q)[KD]) {
    // the weight fragments are the same for every update: an opaque lane index keeps the compiler from hoisting
    // all of them out of the step loop (hundreds of VGPRs)
    int lane = lane0;
    asm volatile("" : "+v"(lane));
    float unused;
    return tile_grad<KD, false>(img, a.net, lane, q, unused);
  };
  for (int64_t tile = wave; tile < a.s.n_tiles; tile += n_waves)
    sim_tile<KD>(a.s, EXPLICIT, a.net.D, lane0, tile * 16, gslot, gslot + kSlotG, z0, traj, tau, last, grad);
}

template <int KD>
__global__ __launch_bounds__(kThreads) void mlp_potential_kernel(TileNet net, const float* __restrict__ x, int64_t n,
                                                                 int64_t ld, int64_t n_tiles,
                                                                 float* __restrict__ value, float* __restrict__ grad) {
  extern __shared__ f32x4 lds4[];
  float* img = reinterpret_cast<float*>(lds4);
  stage_image(lds4, net);
  __syncthreads();
  const int lane0 = threadIdx.x & (kWave - 1), p = lane0 & 15, g = lane0 >> 4;
  const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int D = net.D;
  const int64_t wave = (int64_t)blockIdx.x * kWavesB + wib;
  const int64_t n_waves = (int64_t)gridDim.x * kWavesB;
  for (int64_t tile = wave; tile < n_tiles; tile += n_waves) {
    int lane = lane0;
    asm volatile("" : "+v"(lane));  // opaque: see sde_mlp_kernel
    const int64_t i_raw = tile * 16 + p;
    const bool active = i_raw < n;
    const int64_t i = active ? i_raw : n - 1;
    float xr[KD];
    lane_dims<KD>(x + i * ld, D, g, xr);
    float val;
    const f32x4 ga = tile_grad<KD, true>(img, net, lane, xr, val);
    store_potential(active, i, g, D, val, ga, value, grad);
  }
}

// ---- host ----------------------------------------------------------------------------------------
// dynamic LDS of both kernels: the image and the waves' slots
static size_t lds_bytes(const TileWs& w) {
  return sizeof(float) * ((size_t)w.ip.ia.img_floats + (size_t)kWavesB * kSlot);
}

static int grid_of(int64_t n_tiles) {
  const int64_t need = (n_tiles + kWavesB - 1) / kWavesB, cap = 2 * (int64_t)device_cus();
  return (int)(need < cap ? need : cap);
}

}  // namespace mlps
}  // namespace pdeinv

using namespace pdeinv;
using namespace pdeinv::mlps;

extern "C" int pdeinv_mlp_potential_path(const pdeinv_mlp_shape* s) {
  if (!s || !tile_shape_ok(s)) return 0;
  if (tile_envelope(s)) return 2;
  return pdeinv_mlp_fused_supported(s->dim, s->n_layers, s->width, s->out_features) ? 1 : 0;
}

extern "C" size_t pdeinv_mlp_potential_workspace_bytes(const pdeinv_mlp_shape* s, int64_t n) {
  if (!s || n < 0) return 0;
  const int path = pdeinv_mlp_potential_path(s);
  if (path == 2) return tile_ws(s).total;
  if (path == 1) return mlp_rows_potential_workspace_bytes(s, n);
  return 0;
}

extern "C" int pdeinv_mlp_potential(const pdeinv_mlp_shape* s, const float* params, const float* x, int64_t n,
                                    int64_t ld, float* value, float* grad, void* ws, void* stream) {
  int64_t ldx;
  bool run;
  int rc = potential_checks(
      "mlp_potential", s, tile_shape_ok, [](const pdeinv_mlp_shape* t) { return pdeinv_mlp_potential_path(t) != 0; },
      "shape outside the tile envelope (dim <= 8, width <= 20, n_layers <= 8) and the fused row envelope "
      "(dim <= 16, width <= 1024, n_layers <= 16)",
      params, x, n, ld, value, grad, ws, ldx, run);
  if (rc || !run) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (pdeinv_mlp_potential_path(s) == 1) return mlp_rows_potential(s, params, x, n, ldx, value, grad, ws, st);
  const TileWs w = tile_ws(s);
  float* img = (float*)((char*)ws + w.off_img);
  rc = build_image(w.ip.ia, params, (double*)((char*)ws + w.off_h0), img, st);
  if (rc) return rc;
  const TileNet net = tile_net(w.ip, img);
  const int64_t n_tiles = (n + 15) / 16;
  const dim3 gr((unsigned)grid_of(n_tiles)), bl(kThreads);
  const size_t lds = lds_bytes(w);
  if (w.ip.KD == 1) {
    allow_lds(mlp_potential_kernel<1>);
    hipLaunchKernelGGL(mlp_potential_kernel<1>, gr, bl, lds, st, net, x, n, ldx, n_tiles, value, grad);
  } else {
    allow_lds(mlp_potential_kernel<2>);
    hipLaunchKernelGGL(mlp_potential_kernel<2>, gr, bl, lds, st, net, x, n, ldx, n_tiles, value, grad);
  }
  return check_launch("mlp_potential_kernel");
}

extern "C" int pdeinv_sde_simulate_mlp_supported(const pdeinv_mlp_shape* s) {
  return s && tile_envelope(s) ? 1 : 0;
}

extern "C" size_t pdeinv_sde_simulate_mlp_workspace_bytes(const pdeinv_sde_desc* d, const pdeinv_mlp_shape* s) {
  if (!d || !s || !tile_envelope(s)) return 0;
  return tile_ws(s).total;
}

extern "C" int pdeinv_sde_simulate_mlp(const pdeinv_sde_desc* d, const pdeinv_mlp_shape* s, const float* params,
                                       const float* z0, float* traj, float* tau, float* last, void* ws,
                                       void* stream) {
  SimArgs a{};
  int rc = sim_checked_args("sde_mlp", d, s, tile_shape_ok, tile_envelope,
                            "the learned-potential simulator covers dim <= 8, width <= 20, 1 <= n_layers <= 8", params,
                            z0, traj, tau, last, ws, a.s);
  if (rc || a.s.N == 0) return rc;
  hipStream_t st = (hipStream_t)stream;
  const TileWs w = tile_ws(s);
  float* img = (float*)((char*)ws + w.off_img);
  rc = build_image(w.ip.ia, params, (double*)((char*)ws + w.off_h0), img, st);
  if (rc) return rc;
  a.net = tile_net(w.ip, img);
  const dim3 gr((unsigned)grid_of(a.s.n_tiles)), bl(kThreads);
  const size_t lds = lds_bytes(w);
#define LAUNCH(KD, EX)                                                                                      \
  do {                                                                                                      \
    allow_lds(sde_mlp_kernel<KD, EX>);                                                                      \
    hipLaunchKernelGGL((sde_mlp_kernel<KD, EX>), gr, bl, lds, st, a, z0, traj, tau, last);                  \
  } while (0)
  if (w.ip.KD == 1) {
    if (a.s.noise) LAUNCH(1, true); else LAUNCH(1, false);
  } else {
    if (a.s.noise) LAUNCH(2, true); else LAUNCH(2, false);
  }
#undef LAUNCH
  return check_launch("sde_mlp_kernel");
}
