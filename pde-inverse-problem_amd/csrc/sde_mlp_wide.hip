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
// Simulator layout: that of sde_mlp.hip. The particle on lane & 15; lane group g holds coordinates 4 kk + g of q
// and p; the gradient's C fragment returns to that layout through a per-wave LDS slot; noise is stream_normals
// (the stream of include/pdeinv.h bit for bit); rows leave assembled per wave as whole rows. Blocks are
// persistent (at most one per CU) and step through block tiles of `waves` wave tiles; since the slice hand-over is
// a block barrier, every wave runs every block tile and update (without a tile of its own: on a clamped row, no
// stores). Deterministic: no atomics, and a particle's numbers depend on its global id and its row only.
#include <math.h>

#include "common.h"
#include "mlp_engine.h"
#include "mlp_tile.h"
#include "mlp_tile_wide.h"
#include "sde_common.h"

namespace pdeinv {
namespace mlpw {

struct WideSimArgs {
  int64_t N, poff, ld_z0, n_tiles;
  int32_t n_steps, random_shift;
  float dt, gamma, ns;
  uint32_t k0, k1, ctr_off;
  const float* noise;
  const float* shift_u;
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
  const int lane = threadIdx.x & (kWave - 1), p = lane & 15, g = lane >> 4;
  const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const Regions R = regions(a.net, lds4, wib);
  const int D = a.net.D, M = 2 * D, waves = a.net.waves;
  const int64_t n_btiles = (a.n_tiles + waves - 1) / waves;
  const int64_t tr_stride = a.N * M;
  const float sh_dt = sqrtf(a.dt) * a.ns;
  const bool explicit_noise = a.noise != nullptr;

  for (int64_t bt = blockIdx.x; bt < n_btiles; bt += gridDim.x) {
    const int64_t tile = bt * waves + wib;
    const int64_t row0 = tile * 16, i_raw = row0 + p;
    const bool active = i_raw < a.N;
    const int64_t i = active ? i_raw : a.N - 1;  // inactive lanes compute on a valid row, store nothing
    const int64_t left = a.N - row0;
    const int n_valid = __builtin_amdgcn_readfirstlane((int)(left < 0 ? 0 : (left < 16 ? left : 16)));
    const uint64_t gid = (uint64_t)(a.poff + i);
    const uint32_t plo = (uint32_t)gid, phi = (uint32_t)(gid >> 32);

    float q[2], v[2];
    lane_dims<2>(z0 + i * a.ld_z0, D, g, q);
    lane_dims<2>(z0 + i * a.ld_z0 + D, D, g, v);

    float tau0 = 0.f;
    if (a.random_shift) {
      float u;
      if (a.shift_u) u = a.shift_u[i];
      else u = u32_unit(philox4x32_10(make_uint4(plo, phi, a.ctr_off, 0x80000000u), a.k0, a.k1).x);
      tau0 = u * a.dt;
    }
    const float h_last = a.dt - tau0;

    auto update = [&](float h, float sh, uint32_t s) {
      float unused;
      const f32x4 ga = wide_grad<false>(a.net, f, R.bias4, R.act, lane, q, unused);
      // C fragment (coordinates 4 g + r) -> input layout (coordinate 4 kk + g) through the wave's slot
      *reinterpret_cast<f32x4*>(R.gslot + p * 16 + 4 * g) = ga;
      __builtin_amdgcn_wave_barrier();
      float gr[2];
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) gr[kk] = R.gslot[p * 16 + 4 * kk + g];
      __builtin_amdgcn_wave_barrier();
      float xi[2];
      if (explicit_noise) {
        const float* src = a.noise + ((int64_t)s * a.N + i) * D;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) xi[kk] = 4 * kk + g < D ? src[4 * kk + g] : 0.f;
      } else {
        float n4[8];
        stream_normals<8>(a.k0, a.k1, a.ctr_off + s, plo, phi, n4);
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          const float lo = (g & 1) ? n4[4 * kk + 1] : n4[4 * kk], hi = (g & 1) ? n4[4 * kk + 3] : n4[4 * kk + 2];
          xi[kk] = 4 * kk + g < D ? ((g & 2) ? hi : lo) : 0.f;
        }
      }
      const float gh = a.gamma * h;
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        // p' = p - h*gradU + sqrt(h)*ns*xi - gamma*p*h ; q' = q + h*p'  (sampling_utils.py:17,20)
        const float pn = fmaf(-gh, v[kk], fmaf(sh, xi[kk], fmaf(-h, gr[kk], v[kk])));
        v[kk] = pn;
        q[kk] = fmaf(h, pn, q[kk]);
      }
    };
    auto put = [&](float* dst) {
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        const int k = 4 * kk + g;
        if (k < D) {
          R.zslot[p * M + k] = q[kk];
          R.zslot[p * M + D + k] = v[kk];
        }
      }
      __builtin_amdgcn_wave_barrier();
      store_rows(dst, R.zslot, M, lane, n_valid);
      __builtin_amdgcn_wave_barrier();
    };
    float* tr = traj ? traj + row0 * M : nullptr;
    float* ta = (tau && active && g == 0) ? tau + i : nullptr;

    // update 0: h = tau0 (sample at tau0); updates 1..n-1: h = dt; the final update: h = dt - tau0, lands exactly
    // at T = n*dt (sampling_utils.py:44-46)
    const float sh_0 = sqrtf(tau0) * a.ns, sh_last = sqrtf(h_last) * a.ns;
    for (int s = 0; s <= a.n_steps; ++s) {
      const bool first = s == 0, fin = s == a.n_steps;
      update(first ? tau0 : (fin ? h_last : a.dt), first ? sh_0 : (fin ? sh_last : sh_dt), (uint32_t)s);
      if (!fin) {
        if (tr) put(tr + (int64_t)s * tr_stride);
        if (ta) __builtin_nontemporal_store(tau_value(tau0, s, a.dt), ta + (int64_t)s * a.N);
      } else if (last) {
        put(last + row0 * M);
      }
    }
  }
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
    if (active) {
      if (value && g == 0) value[i] = val;
      if (grad) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (4 * g + r < D) grad[i * D + 4 * g + r] = ga[r];
      }
    }
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
  PDEINV_REQUIRE(s != nullptr, PDEINV_ERR_INVALID, "mlp_potential_wide: null shape");
  PDEINV_REQUIRE(shape_ok(s), PDEINV_ERR_INVALID,
                 "mlp_potential_wide: dim, n_layers, width and out_features must be >= 1");
  PDEINV_REQUIRE(pdeinv_sde_simulate_mlp_wide_supported(s), PDEINV_ERR_UNSUPPORTED,
                 "mlp_potential_wide: the wide tile covers " WIDE_ENVELOPE_TEXT);
  PDEINV_REQUIRE(n >= 0, PDEINV_ERR_INVALID, "mlp_potential_wide: n < 0");
  const int64_t ldx = ld ? ld : s->dim;
  PDEINV_REQUIRE(ldx >= s->dim, PDEINV_ERR_INVALID, "mlp_potential_wide: ld < dim");
  if (n == 0 || (value == nullptr && grad == nullptr)) return PDEINV_OK;
  PDEINV_REQUIRE(params != nullptr && x != nullptr, PDEINV_ERR_INVALID, "mlp_potential_wide: params / x is null");
  PDEINV_REQUIRE(ws != nullptr && (uintptr_t)ws % 256 == 0, PDEINV_ERR_INVALID,
                 "mlp_potential_wide: workspace is null or not 256-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const WideNet net = net_of(s, (const float*)ws);
  int rc = wide_build_image(net, params, (float*)ws, st);
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
  PDEINV_REQUIRE(d != nullptr, PDEINV_ERR_INVALID, "sde_mlp_wide: null descriptor");
  PDEINV_REQUIRE(s != nullptr, PDEINV_ERR_INVALID, "sde_mlp_wide: null shape");
  PDEINV_REQUIRE(d->potential.kind == PDEINV_POT_MLP, PDEINV_ERR_INVALID,
                 "sde_mlp_wide: potential kind must be PDEINV_POT_MLP");
  PDEINV_REQUIRE(shape_ok(s), PDEINV_ERR_INVALID,
                 "sde_mlp_wide: dim, n_layers, width and out_features must be >= 1");
  PDEINV_REQUIRE(pdeinv_sde_simulate_mlp_wide_supported(s), PDEINV_ERR_UNSUPPORTED,
                 "sde_mlp_wide: the wide learned-potential simulator covers " WIDE_ENVELOPE_TEXT);
  PDEINV_REQUIRE(d->dim == s->dim, PDEINV_ERR_INVALID, "sde_mlp_wide: descriptor and shape disagree on dim");
  pdeinv_sde_desc dd = *d;  // the shared descriptor checks; the potential's fields are not read
  dd.potential = pdeinv_potential{};
  dd.potential.kind = PDEINV_POT_NONE;
  SdeArgs sa;
  int rc = build_args(&dd, sa);
  if (rc) return rc;
  if (sa.N == 0) return PDEINV_OK;
  PDEINV_REQUIRE(z0 != nullptr && params != nullptr, PDEINV_ERR_INVALID, "sde_mlp_wide: z0 / params is null");
  PDEINV_REQUIRE(ws != nullptr && (uintptr_t)ws % 256 == 0, PDEINV_ERR_INVALID,
                 "sde_mlp_wide: workspace is null or not 256-byte aligned");
  const size_t va = (s->dim % 2 == 0) ? 16 : 8;
  PDEINV_REQUIRE(aligned(traj, va) && aligned(last, va) && aligned(tau, 4), PDEINV_ERR_INVALID,
                 "sde_mlp_wide: traj/last must be 16-byte (even dim) or 8-byte (odd dim) aligned");
  hipStream_t st = (hipStream_t)stream;
  const WideNet net = net_of(s, (const float*)ws);
  rc = wide_build_image(net, params, (float*)ws, st);
  if (rc) return rc;
  WideSimArgs a{};
  a.N = sa.N; a.poff = sa.poff; a.ld_z0 = sa.ld_z0;
  a.n_tiles = (sa.N + 15) / 16;
  a.n_steps = sa.n_steps; a.random_shift = sa.random_shift;
  a.dt = sa.dt; a.gamma = sa.gamma; a.ns = sa.ns;
  a.k0 = sa.k0; a.k1 = sa.k1; a.ctr_off = sa.ctr_off;
  a.noise = sa.noise; a.shift_u = sa.shift_u;
  a.net = net;
  const dim3 gr((unsigned)grid_of(a.n_tiles, net.waves)), bl((unsigned)(net.waves * kWave));
  allow_lds(sde_mlp_wide_kernel);
  hipLaunchKernelGGL(sde_mlp_wide_kernel, gr, bl, wide_lds_bytes(net), st, a, z0, traj, tau, last);
  return check_launch("sde_mlp_wide_kernel");
}
