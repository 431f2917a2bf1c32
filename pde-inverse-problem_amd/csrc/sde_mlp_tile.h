// sde_mlp_tile.h — what the two learned-potential simulators (sde_mlp.hip: width <= 20, sde_mlp_wide.hip: width
// 21..256) share: utils/sampling_utils.py:6-52 (update_step, underdamped_langevin_dynamics_scan) for one tile of
// 16 particles, around a gradient that the caller supplies; the potential kernels' epilogue; the host checks of
// the four entry points. The files keep what differs: how a tile gets its gradient and how waves map to tiles.
//
// Simulator layout. A wave owns the 16 particles of a tile: the particle on lane & 15, and lane group g = lane >> 4
// holds coordinates 4 kk + g of q and p (lane_dims), which is the B operand of the first product. q and p stay in
// registers across all n_steps + 1 updates. The gradient leaves the last backward product as a C fragment
// (coordinates 4 g + r of the particle): one 1 KiB per-wave LDS slot turns it back into the input layout (one
// 16-byte write, KD 4-byte reads per lane and update) — the only lane traffic of an update. Noise: every lane group
// draws its particle's Philox block kk (stream_normals: the stream of include/pdeinv.h bit for bit) and keeps
// normal 4 kk + g. Stores: the tile's 16 rows of 2d floats are assembled in a second per-wave LDS slot and leave as
// 16-byte (even d) or 8-byte (odd d) nontemporal pieces of whole rows. Deterministic: no atomics, and a particle's
// numbers depend on its global id and its row only (MFMA columns do not mix), so any sharding of the particles
// over calls gives the same bits.
#pragma once
#include <math.h>

#include <string>

#include "common.h"
#include "mlp_tile.h"
#include "sde_common.h"

namespace pdeinv {
namespace mlpq {

constexpr int kSlotG = 16 * 16;  // gradient slot of a wave: [particle][16 coordinates]
constexpr int kSlotZ = 16 * 16;  // row slot of a wave: [particle][2d], d <= 8

// The simulator's kernel arguments but for the net.
struct TileSimArgs {
  int64_t N, poff, ld_z0, n_tiles;
  int32_t n_steps, random_shift;
  float dt, gamma, ns;
  uint32_t k0, k1, ctr_off;
  const float* noise;
  const float* shift_u;
};

// The tile's rows [16][M] (M = 2d floats, assembled in `slot`) -> dst, whole rows, n_valid of them: 16-byte pieces
// when M % 4 == 0 (rows then start on 16-byte boundaries), 8-byte pieces otherwise (M is even).
__device__ __forceinline__ void store_rows(float* dst, const float* slot, int M, int lane, int n_valid) {
  const int nf = n_valid * M;
  if ((M & 3) == 0) {
    const int c = lane;  // 4 M <= 64 chunks
    if (4 * c < nf)
      __builtin_nontemporal_store(*reinterpret_cast<const f32x4*>(slot + 4 * c), reinterpret_cast<f32x4*>(dst) + c);
  } else {
#pragma unroll
    for (int it = 0; it < 2; ++it) {  // 8 M <= 112 chunks
      const int c = lane + 64 * it;
      if (2 * c < nf)
        __builtin_nontemporal_store(*reinterpret_cast<const f32x2*>(slot + 2 * c), reinterpret_cast<f32x2*>(dst) + c);
    }
  }
}

// All n_steps + 1 updates of the tile of rows row0 .. row0 + 15, from the load of z0 to the last store. grad(q):
// the C fragment of grad V at the lanes' coordinates q (register r of lane (particle, g) is dV / dx_{4 g + r}).
// gslot / zslot: the wave's kSlotG / kSlotZ floats of LDS. A tile at or past the end (row0 >= N) computes on the
// clamped last row and stores nothing.
template <int KD, class Grad>
__device__ __forceinline__ void sim_tile(const TileSimArgs& a, bool explicit_noise, int D, int lane, int64_t row0,
                                         float* gslot, float* zslot, const float* __restrict__ z0,
                                         float* __restrict__ traj, float* __restrict__ tau, float* __restrict__ last,
                                         Grad&& grad) {
  const int p = lane & 15, g = lane >> 4, M = 2 * D;
  const int64_t tr_stride = a.N * M;
  const float sh_dt = sqrtf(a.dt) * a.ns;
  const int64_t i_raw = row0 + p;
  const bool active = i_raw < a.N;
  const int64_t i = active ? i_raw : a.N - 1;  // inactive lanes compute on a valid row, store nothing
  const int64_t left = a.N - row0;
  const int n_valid = __builtin_amdgcn_readfirstlane((int)(left < 0 ? 0 : (left < 16 ? left : 16)));
  const uint64_t gid = (uint64_t)(a.poff + i);
  const uint32_t plo = (uint32_t)gid, phi = (uint32_t)(gid >> 32);

  float q[KD], v[KD];
  lane_dims<KD>(z0 + i * a.ld_z0, D, g, q);
  lane_dims<KD>(z0 + i * a.ld_z0 + D, D, g, v);

  float tau0 = 0.f;
  if (a.random_shift) {
    float u;
    if (a.shift_u) u = a.shift_u[i];
    else u = u32_unit(philox4x32_10(make_uint4(plo, phi, a.ctr_off, 0x80000000u), a.k0, a.k1).x);
    tau0 = u * a.dt;
  }
  const float h_last = a.dt - tau0;

  auto update = [&](float h, float sh, uint32_t s) {
    const f32x4 ga = grad(q);
    // C fragment (coordinates 4 g + r) -> input layout (coordinate 4 kk + g) through the wave's slot
    *reinterpret_cast<f32x4*>(gslot + p * 16 + 4 * g) = ga;
    __builtin_amdgcn_wave_barrier();
    float gr[KD];
#pragma unroll
    for (int kk = 0; kk < KD; ++kk) gr[kk] = gslot[p * 16 + 4 * kk + g];
    __builtin_amdgcn_wave_barrier();
    float xi[KD];
    if (explicit_noise) {
      const float* src = a.noise + ((int64_t)s * a.N + i) * D;
#pragma unroll
      for (int kk = 0; kk < KD; ++kk) xi[kk] = 4 * kk + g < D ? src[4 * kk + g] : 0.f;
    } else {
      float n4[4 * KD];
      stream_normals<4 * KD>(a.k0, a.k1, a.ctr_off + s, plo, phi, n4);
#pragma unroll
      for (int kk = 0; kk < KD; ++kk) {
        const float lo = (g & 1) ? n4[4 * kk + 1] : n4[4 * kk], hi = (g & 1) ? n4[4 * kk + 3] : n4[4 * kk + 2];
        xi[kk] = 4 * kk + g < D ? ((g & 2) ? hi : lo) : 0.f;
      }
    }
    const float gh = a.gamma * h;
#pragma unroll
    for (int kk = 0; kk < KD; ++kk) {
      // p' = p - h*gradU + sqrt(h)*ns*xi - gamma*p*h ; q' = q + h*p'  (sampling_utils.py:17,20)
      const float pn = fmaf(-gh, v[kk], fmaf(sh, xi[kk], fmaf(-h, gr[kk], v[kk])));
      v[kk] = pn;
      q[kk] = fmaf(h, pn, q[kk]);
    }
  };
  auto put = [&](float* dst) {
#pragma unroll
    for (int kk = 0; kk < KD; ++kk) {
      const int k = 4 * kk + g;
      if (k < D) {
        zslot[p * M + k] = q[kk];
        zslot[p * M + D + k] = v[kk];
      }
    }
    __builtin_amdgcn_wave_barrier();
    store_rows(dst, zslot, M, lane, n_valid);
    __builtin_amdgcn_wave_barrier();
  };
  float* tr = traj ? traj + row0 * M : nullptr;
  float* ta = (tau && active && g == 0) ? tau + i : nullptr;

  // update 0: h = tau0 (sample at tau0); updates 1..n-1: h = dt; the final update: h = dt - tau0, lands exactly
  // at T = n*dt (sampling_utils.py:44-46). One loop body: the gradient's code is instantiated once.
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

// The potential kernels' epilogue: V and the gradient's C fragment (coordinates 4 g + r) of particle i.
__device__ __forceinline__ void store_potential(bool active, int64_t i, int g, int D, float val, f32x4 ga,
                                                float* __restrict__ value, float* __restrict__ grad) {
  if (active) {
    if (value && g == 0) value[i] = val;
    if (grad) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (4 * g + r < D) grad[i * D + 4 * g + r] = ga[r];
    }
  }
}

// ---- host ----------------------------------------------------------------------------------------
typedef bool (*ShapeTest)(const pdeinv_mlp_shape*);

// The checks of a simulator entry point `name` (the messages' prefix), before any device call, and its arguments
// from the descriptor. envelope_text: what the entry point covers. a.N == 0 on PDEINV_OK: nothing to do, and the
// pointers are unchecked.
inline int sim_checked_args(const std::string& name, const pdeinv_sde_desc* d, const pdeinv_mlp_shape* s,
                            ShapeTest shape_ok, ShapeTest envelope, const char* envelope_text, const float* params,
                            const float* z0, const float* traj, const float* tau, const float* last, const void* ws,
                            TileSimArgs& a) {
  a = TileSimArgs{};
  PDEINV_REQUIRE(d != nullptr, PDEINV_ERR_INVALID, name + ": null descriptor");
  PDEINV_REQUIRE(s != nullptr, PDEINV_ERR_INVALID, name + ": null shape");
  PDEINV_REQUIRE(d->potential.kind == PDEINV_POT_MLP, PDEINV_ERR_INVALID,
                 name + ": potential kind must be PDEINV_POT_MLP");
  PDEINV_REQUIRE(shape_ok(s), PDEINV_ERR_INVALID, name + ": dim, n_layers, width and out_features must be >= 1");
  PDEINV_REQUIRE(envelope(s), PDEINV_ERR_UNSUPPORTED, name + ": " + envelope_text);
  PDEINV_REQUIRE(d->dim == s->dim, PDEINV_ERR_INVALID, name + ": descriptor and shape disagree on dim");
  SdeArgs sa;
  const int rc = build_args_without_potential(d, sa);
  if (rc) return rc;
  if (sa.N == 0) return PDEINV_OK;
  PDEINV_REQUIRE(z0 != nullptr && params != nullptr, PDEINV_ERR_INVALID, name + ": z0 / params is null");
  PDEINV_REQUIRE(ws != nullptr && (uintptr_t)ws % 256 == 0, PDEINV_ERR_INVALID,
                 name + ": workspace is null or not 256-byte aligned");
  const size_t va = (s->dim % 2 == 0) ? 16 : 8;
  PDEINV_REQUIRE(aligned(traj, va) && aligned(last, va) && aligned(tau, 4), PDEINV_ERR_INVALID,
                 name + ": traj/last must be 16-byte (even dim) or 8-byte (odd dim) aligned");
  a.N = sa.N; a.poff = sa.poff; a.ld_z0 = sa.ld_z0;
  a.n_tiles = (sa.N + 15) / 16;
  a.n_steps = sa.n_steps; a.random_shift = sa.random_shift;
  a.dt = sa.dt; a.gamma = sa.gamma; a.ns = sa.ns;
  a.k0 = sa.k0; a.k1 = sa.k1; a.ctr_off = sa.ctr_off;
  a.noise = sa.noise; a.shift_u = sa.shift_u;
  return PDEINV_OK;
}

// The checks of a potential entry point `name`, before any device call. ldx: the row stride of x. run: false on
// PDEINV_OK when there is nothing to do (no rows or no output), and then the pointers are unchecked.
inline int potential_checks(const std::string& name, const pdeinv_mlp_shape* s, ShapeTest shape_ok,
                            ShapeTest envelope, const char* envelope_text, const float* params, const float* x,
                            int64_t n, int64_t ld, const float* value, const float* grad, const void* ws,
                            int64_t& ldx, bool& run) {
  run = false;
  PDEINV_REQUIRE(s != nullptr, PDEINV_ERR_INVALID, name + ": null shape");
  PDEINV_REQUIRE(shape_ok(s), PDEINV_ERR_INVALID, name + ": dim, n_layers, width and out_features must be >= 1");
  PDEINV_REQUIRE(envelope(s), PDEINV_ERR_UNSUPPORTED, name + ": " + envelope_text);
  PDEINV_REQUIRE(n >= 0, PDEINV_ERR_INVALID, name + ": n < 0");
  ldx = ld ? ld : s->dim;
  PDEINV_REQUIRE(ldx >= s->dim, PDEINV_ERR_INVALID, name + ": ld < dim");
  if (n == 0 || (value == nullptr && grad == nullptr)) return PDEINV_OK;
  PDEINV_REQUIRE(params != nullptr && x != nullptr, PDEINV_ERR_INVALID, name + ": params / x is null");
  PDEINV_REQUIRE(ws != nullptr && (uintptr_t)ws % 256 == 0, PDEINV_ERR_INVALID,
                 name + ": workspace is null or not 256-byte aligned");
  run = true;
  return PDEINV_OK;
}

}  // namespace mlpq
}  // namespace pdeinv
