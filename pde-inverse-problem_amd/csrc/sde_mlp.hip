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
// Simulator layout. A wave owns 16 particles per tile: the particle on lane & 15, and lane group g = lane >> 4
// holds coordinates 4 kk + g of q and p (lane_dims), which is the B operand of the first product. q and p stay in
// registers across all n_steps + 1 updates. The gradient leaves the last backward product as a C fragment
// (coordinates 4 g + r of the particle): one 1 KiB per-wave LDS slot turns it back into the input layout (one
// 16-byte write, KD 4-byte reads per lane and update) — the only lane traffic of an update. Noise: every lane group
// draws its particle's Philox block kk (stream_normals: the stream of include/pdeinv.h bit for bit) and keeps
// normal 4 kk + g. Stores: the tile's 16 rows of 2d floats are assembled in a second per-wave LDS slot and leave as
// 16-byte (even d) or 8-byte (odd d) nontemporal pieces of whole rows. Deterministic: no atomics, and a particle's
// numbers depend on its global id and its row only (MFMA columns do not mix), so any sharding of the particles
// over calls gives the same bits.
#include <math.h>

#include "common.h"
#include "mlp_engine.h"
#include "mlp_tile.h"
#include "sde_common.h"

namespace pdeinv {
namespace mlps {

using namespace mlpq;

constexpr int kWavesB = 8;                 // waves per block: two blocks per CU = 4 waves per SIMD
constexpr int kThreads = kWavesB * kWave;
constexpr int kSlotG = 16 * 16;            // gradient slot: [particle][16 coordinates]
constexpr int kSlotZ = 16 * 2 * 8;         // row slot: [particle][2d], d <= 8
constexpr int kSlot = kSlotG + kSlotZ;     // floats per wave

struct SimArgs {
  int64_t N, poff, ld_z0, n_tiles;
  int32_t n_steps, random_shift;
  float dt, gamma, ns;
  uint32_t k0, k1, ctr_off;
  const float* noise;
  const float* shift_u;
  TileNet net;
};

// The tile's rows [16][M] (M = 2d floats, assembled in `slot`) -> dst, whole rows, n_valid of them: 16-byte pieces
// when M % 4 == 0 (rows then start on 16-byte boundaries), 8-byte pieces otherwise (M is even).
__device__ __forceinline__ void store_tile(float* dst, const float* slot, int M, int lane, int n_valid) {
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

template <int KD, bool EXPLICIT>
__global__ __launch_bounds__(kThreads) void sde_mlp_kernel(SimArgs a, const float* __restrict__ z0,
                                                           float* __restrict__ traj, float* __restrict__ tau,
                                                           float* __restrict__ last) {
  extern __shared__ f32x4 lds4[];
  float* img = reinterpret_cast<float*>(lds4);
  stage_image(lds4, a.net);
  __syncthreads();
  const int lane0 = threadIdx.x & (kWave - 1), p = lane0 & 15, g = lane0 >> 4;
  const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  float* gslot = img + a.net.img_floats + wib * kSlot;
  float* zslot = gslot + kSlotG;
  const int D = a.net.D, M = 2 * D;
  const int64_t wave = (int64_t)blockIdx.x * kWavesB + wib;
  const int64_t n_waves = (int64_t)gridDim.x * kWavesB;
  const int64_t tr_stride = a.N * M;
  const float sh_dt = sqrtf(a.dt) * a.ns;

  for (int64_t tile = wave; tile < a.n_tiles; tile += n_waves) {
    const int64_t row0 = tile * 16, i_raw = row0 + p;
    const bool active = i_raw < a.N;
    const int64_t i = active ? i_raw : a.N - 1;  // inactive lanes compute on a valid row, store nothing
    const int n_valid = __builtin_amdgcn_readfirstlane((int)((a.N - row0) < 16 ? (a.N - row0) : 16));
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
      // the weight fragments are the same for every update: an opaque lane index keeps the compiler from hoisting
      // all of them out of the step loop (hundreds of VGPRs)
      int lane = lane0;
      asm volatile("" : "+v"(lane));
      float unused;
      const f32x4 ga = tile_grad<KD, false>(img, a.net, lane, q, unused);
      // C fragment (coordinates 4 g + r) -> input layout (coordinate 4 kk + g) through the wave's slot
      *reinterpret_cast<f32x4*>(gslot + p * 16 + 4 * g) = ga;
      __builtin_amdgcn_wave_barrier();
      float gr[KD];
#pragma unroll
      for (int kk = 0; kk < KD; ++kk) gr[kk] = gslot[p * 16 + 4 * kk + g];
      __builtin_amdgcn_wave_barrier();
      float xi[KD];
      if constexpr (EXPLICIT) {
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
      store_tile(dst, zslot, M, lane0, n_valid);
      __builtin_amdgcn_wave_barrier();
    };
    float* tr = traj ? traj + row0 * M : nullptr;
    float* ta = (tau && active && g == 0) ? tau + i : nullptr;

    // update 0: h = tau0 (sample at tau0); updates 1..n-1: h = dt; the final update: h = dt - tau0, lands exactly
    // at T = n*dt (sampling_utils.py:44-46). One loop body: the tile code is instantiated once.
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
  PDEINV_REQUIRE(s != nullptr, PDEINV_ERR_INVALID, "mlp_potential: null shape");
  PDEINV_REQUIRE(tile_shape_ok(s), PDEINV_ERR_INVALID,
                 "mlp_potential: dim, n_layers, width and out_features must be >= 1");
  const int path = pdeinv_mlp_potential_path(s);
  PDEINV_REQUIRE(path != 0, PDEINV_ERR_UNSUPPORTED,
                 "mlp_potential: shape outside the tile envelope (dim <= 8, width <= 20, n_layers <= 8) and the "
                 "fused row envelope (dim <= 16, width <= 1024, n_layers <= 16)");
  PDEINV_REQUIRE(n >= 0, PDEINV_ERR_INVALID, "mlp_potential: n < 0");
  const int64_t ldx = ld ? ld : s->dim;
  PDEINV_REQUIRE(ldx >= s->dim, PDEINV_ERR_INVALID, "mlp_potential: ld < dim");
  if (n == 0 || (value == nullptr && grad == nullptr)) return PDEINV_OK;
  PDEINV_REQUIRE(params != nullptr && x != nullptr, PDEINV_ERR_INVALID, "mlp_potential: params / x is null");
  PDEINV_REQUIRE(ws != nullptr && (uintptr_t)ws % 256 == 0, PDEINV_ERR_INVALID,
                 "mlp_potential: workspace is null or not 256-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (path == 1) return mlp_rows_potential(s, params, x, n, ldx, value, grad, ws, st);
  const TileWs w = tile_ws(s);
  float* img = (float*)((char*)ws + w.off_img);
  int rc = build_image(w.ip.ia, params, (double*)((char*)ws + w.off_h0), img, st);
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
  PDEINV_REQUIRE(d != nullptr, PDEINV_ERR_INVALID, "sde_mlp: null descriptor");
  PDEINV_REQUIRE(s != nullptr, PDEINV_ERR_INVALID, "sde_mlp: null shape");
  PDEINV_REQUIRE(d->potential.kind == PDEINV_POT_MLP, PDEINV_ERR_INVALID,
                 "sde_mlp: potential kind must be PDEINV_POT_MLP");
  PDEINV_REQUIRE(tile_shape_ok(s), PDEINV_ERR_INVALID,
                 "sde_mlp: dim, n_layers, width and out_features must be >= 1");
  PDEINV_REQUIRE(tile_envelope(s), PDEINV_ERR_UNSUPPORTED,
                 "sde_mlp: the learned-potential simulator covers dim <= 8, width <= 20, 1 <= n_layers <= 8");
  PDEINV_REQUIRE(d->dim == s->dim, PDEINV_ERR_INVALID, "sde_mlp: descriptor and shape disagree on dim");
  pdeinv_sde_desc dd = *d;  // the shared descriptor checks; the potential's fields are not read
  dd.potential = pdeinv_potential{};
  dd.potential.kind = PDEINV_POT_NONE;
  SdeArgs sa;
  int rc = build_args(&dd, sa);
  if (rc) return rc;
  if (sa.N == 0) return PDEINV_OK;
  PDEINV_REQUIRE(z0 != nullptr && params != nullptr, PDEINV_ERR_INVALID, "sde_mlp: z0 / params is null");
  PDEINV_REQUIRE(ws != nullptr && (uintptr_t)ws % 256 == 0, PDEINV_ERR_INVALID,
                 "sde_mlp: workspace is null or not 256-byte aligned");
  const size_t va = (s->dim % 2 == 0) ? 16 : 8;
  PDEINV_REQUIRE(aligned(traj, va) && aligned(last, va) && aligned(tau, 4), PDEINV_ERR_INVALID,
                 "sde_mlp: traj/last must be 16-byte (even dim) or 8-byte (odd dim) aligned");
  hipStream_t st = (hipStream_t)stream;
  const TileWs w = tile_ws(s);
  float* img = (float*)((char*)ws + w.off_img);
  rc = build_image(w.ip.ia, params, (double*)((char*)ws + w.off_h0), img, st);
  if (rc) return rc;
  SimArgs a{};
  a.N = sa.N; a.poff = sa.poff; a.ld_z0 = sa.ld_z0;
  a.n_tiles = (sa.N + 15) / 16;
  a.n_steps = sa.n_steps; a.random_shift = sa.random_shift;
  a.dt = sa.dt; a.gamma = sa.gamma; a.ns = sa.ns;
  a.k0 = sa.k0; a.k1 = sa.k1; a.ctr_off = sa.ctr_off;
  a.noise = sa.noise; a.shift_u = sa.shift_u;
  a.net = tile_net(w.ip, img);
  const dim3 gr((unsigned)grid_of(a.n_tiles)), bl(kThreads);
  const size_t lds = lds_bytes(w);
#define LAUNCH(KD, EX)                                                                                      \
  do {                                                                                                      \
    allow_lds(sde_mlp_kernel<KD, EX>);                                                                      \
    hipLaunchKernelGGL((sde_mlp_kernel<KD, EX>), gr, bl, lds, st, a, z0, traj, tau, last);                  \
  } while (0)
  if (w.ip.KD == 1) {
    if (a.noise) LAUNCH(1, true); else LAUNCH(1, false);
  } else {
    if (a.noise) LAUNCH(2, true); else LAUNCH(2, false);
  }
#undef LAUNCH
  return check_launch("sde_mlp_kernel");
}
