// sde_mf_mlp.hip — the learned interaction Phi_theta = V_hypothesis (core/model.py:32-62) of the kinetic
// McKean–Vlasov system as a force and as the simulator's interaction (gfx950):
//   pdeinv_mf_mlp_force   F_i = (1/m) sum_{j<m} grad Phi_theta(x_i - r_j) for items x [n] against references r [m]
//                         (the pairwise mean of kinetic_mckean_vlasov.py:20-23, x_minus_ref; the self pair counts);
//   pdeinv_mf_mlp_step    one update of utils/sampling_utils.py:6-22 for this call's particles with that force,
//                         the references being the gathered positions of the whole ensemble (all ranks);
//   pdeinv_mf_mlp_prepare the weight image, once per simulate, into the workspace the steps read.
//
// Force. The pair-force kernel of mlp_pairs_mfma.hip (mlpq::pair_force_partials, which is also the gbar pass of the
// KMV residual) with one set of items against one set of references: a wave per (item, chunk of kChunk references by
// reference index), mlpq::tile_grad on each 16-pair tile, the unit's D sums to gpart[item][chunk]. No atomics. An
// item's numbers depend on its own row and on the reference set in its order only: the chunk grid is fixed by the
// reference index, not by n, by the items that share the call, or by the launch grid.
//
// Reduce / step. The chunk partials of an item are summed in chunk order in fp64 and scaled by 1/m
// (mlpq::reduce_chunks). The batch entry does that in the small kernel of mlpq::pair_force_reduce; the simulator's
// step does it at the head of the update kernel instead of through a force array: the update is one thread per
// particle with 2d floats of state, so the fused form saves a launch and a round trip of [N, d] per update and costs
// nothing (n_ch <= 20 partials per coordinate at N = 5000). Both call the same function, so the step's force is the
// batch entry's bit for bit. The update itself is mf_step_kernel's (sde.hip): the Philox stream of include/pdeinv.h
// through stream_normals with the global id as the counter, explicit d_noise honoured, the shared clock tau0 of the
// ensemble (shared_tau0_host), h = tau0 / dt / dt - tau0.
#include <math.h>

#include "common.h"
#include "mlp_tile.h"
#include "sde_common.h"

namespace pdeinv {
namespace mlpmf {

using namespace mlpq;

struct StepArgs {
  int64_t N, poff, ld_z;
  int32_t s, n_steps, n_ch;
  float dt, gamma, ns, tau0;
  uint32_t k0, k1, ctr_off;
  const float* noise;
  double inv_m;
};

// One update of particle i: the force from its chunk partials, then mf_step_kernel's update (sde.hip).
template <int D>
__global__ __launch_bounds__(kBlock) void mf_mlp_step_kernel(StepArgs a, const float* __restrict__ gpart,
                                                             const float* zin, float* zout, float* tau_row) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= a.N) return;
  float F[D], q[D], v[D], xi[D];
#pragma unroll
  for (int k = 0; k < D; ++k) F[k] = reduce_chunks(gpart, i, a.n_ch, D, k, a.inv_m);
#pragma unroll
  for (int k = 0; k < D; ++k) {
    q[k] = zin[i * a.ld_z + k];
    v[k] = zin[i * a.ld_z + D + k];
  }
  if (a.noise) {
    const float* src = a.noise + ((int64_t)a.s * a.N + i) * D;
#pragma unroll
    for (int k = 0; k < D; ++k) xi[k] = src[k];
  } else {
    const uint64_t gid = (uint64_t)(a.poff + i);
    stream_normals<D>(a.k0, a.k1, a.ctr_off + (uint32_t)a.s, (uint32_t)gid, (uint32_t)(gid >> 32), xi);
  }
  const float h = (a.s == 0) ? a.tau0 : ((a.s == a.n_steps) ? a.dt - a.tau0 : a.dt);
  const float sh = sqrtf(h) * a.ns;
  const float gh = a.gamma * h;
#pragma unroll
  for (int k = 0; k < D; ++k) {
    // p' = p - h*F + sqrt(h)*ns*xi - gamma*p*h ; q' = q + h*p'  (sampling_utils.py:17,20)
    const float pn = fmaf(-gh, v[k], fmaf(sh, xi[k], fmaf(-h, F[k], v[k])));
    zout[i * 2 * D + D + k] = pn;
    zout[i * 2 * D + k] = fmaf(h, pn, q[k]);
  }
  if (tau_row) tau_row[i] = tau_value(a.tau0, a.s, a.dt);
}

// ---- host ----------------------------------------------------------------------------------------
static const char* const kEnvelope =
    "mf_mlp: the learned-interaction kernels cover dim <= 8, width <= 20, 1 <= n_layers <= 8";

// workspace: the tile kernels' [image | h0y0] and gpart (n items x n_ch x D floats)
struct Ws {
  TileWs t;
  int n_ch;
  size_t off_gpart, total;
};
static Ws ws_plan(const pdeinv_mlp_shape* s, int64_t n, int64_t m) {
  Ws w{};
  w.t = tile_ws(s);
  w.n_ch = pair_chunks(m);
  w.total = w.t.total;
  w.off_gpart = take(w.total, sizeof(float) * (size_t)n * (size_t)w.n_ch * (size_t)s->dim);
  return w;
}

// the image of this call's parameters into the workspace
static int image_into(const Ws& w, void* ws, const float* params, hipStream_t st) {
  return build_image(w.t.ip.ia, params, (double*)((char*)ws + w.t.off_h0), (float*)((char*)ws + w.t.off_img), st);
}

// the chunk partials of items x [n] against references r [m] into the workspace's gpart (the image is in place)
static int force_partials(const Ws& w, void* ws, const float* x, int64_t n, int64_t ldx, const float* r, int64_t m,
                          int64_t ldr, hipStream_t st) {
  PairForce f{};
  f.x = x; f.r = r;
  f.ldx = ldx; f.ldr = ldr;
  f.n_sets = 1; f.n = n; f.m = m;
  f.gpart = (float*)((char*)ws + w.off_gpart);
  f.net = tile_net(w.t.ip, (const float*)((char*)ws + w.t.off_img));
  return pair_force_partials(f, st);
}

}  // namespace mlpmf
}  // namespace pdeinv

using namespace pdeinv;
using namespace pdeinv::mlpmf;

extern "C" int pdeinv_mf_mlp_supported(const pdeinv_mlp_shape* s) { return s && tile_envelope(s) ? 1 : 0; }

extern "C" size_t pdeinv_mf_mlp_workspace_bytes(const pdeinv_mlp_shape* s, int64_t n, int64_t m) {
  if (!s || !tile_envelope(s) || n < 0 || m < 1) return 0;
  return ws_plan(s, n, m).total;
}

// the checks shared by the three entry points (before any device call)
static int check_shape_ws(const pdeinv_mlp_shape* s, const void* ws, bool need_ws) {
  PDEINV_REQUIRE(s != nullptr, PDEINV_ERR_INVALID, "mf_mlp: null shape");
  PDEINV_REQUIRE(tile_shape_ok(s), PDEINV_ERR_INVALID, "mf_mlp: dim, n_layers, width and out_features must be >= 1");
  PDEINV_REQUIRE(tile_envelope(s), PDEINV_ERR_UNSUPPORTED, kEnvelope);
  if (need_ws)
    PDEINV_REQUIRE(ws != nullptr && (uintptr_t)ws % 256 == 0, PDEINV_ERR_INVALID,
                   "mf_mlp: workspace is null or not 256-byte aligned");
  return PDEINV_OK;
}

extern "C" int pdeinv_mf_mlp_prepare(const pdeinv_mlp_shape* s, const float* params, void* ws, void* stream) {
  int rc = check_shape_ws(s, ws, true);
  if (rc) return rc;
  PDEINV_REQUIRE(params != nullptr && aligned(params, 4), PDEINV_ERR_INVALID,
                 "mf_mlp_prepare: params is null or unaligned");
  // (the image and h0y0 offsets do not depend on n, m)
  return image_into(ws_plan(s, 0, 1), ws, params, (hipStream_t)stream);
}

extern "C" int pdeinv_mf_mlp_force(const pdeinv_mlp_shape* s, const float* params, const float* x, int64_t n,
                                   int64_t ldx, const float* r, int64_t m, int64_t ldr, float* force, void* ws,
                                   void* stream) {
  int rc = check_shape_ws(s, ws, false);
  if (rc) return rc;
  PDEINV_REQUIRE(n >= 0, PDEINV_ERR_INVALID, "mf_mlp_force: n < 0");
  PDEINV_REQUIRE(m >= 1, PDEINV_ERR_INVALID, "mf_mlp_force: m < 1 (the mean over an empty reference set)");
  const int64_t lx = ldx ? ldx : s->dim, lr = ldr ? ldr : s->dim;
  PDEINV_REQUIRE(lx >= s->dim && lr >= s->dim, PDEINV_ERR_INVALID, "mf_mlp_force: ldx / ldr < dim");
  if (n == 0) return PDEINV_OK;
  PDEINV_REQUIRE(params != nullptr && x != nullptr && r != nullptr && force != nullptr, PDEINV_ERR_INVALID,
                 "mf_mlp_force: params / x / r / force is null");
  PDEINV_REQUIRE(aligned(params, 4) && aligned(x, 4) && aligned(r, 4) && aligned(force, 4), PDEINV_ERR_INVALID,
                 "mf_mlp_force: pointers must be 4-byte aligned");
  rc = check_shape_ws(s, ws, true);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const Ws w = ws_plan(s, n, m);
  rc = image_into(w, ws, params, st);
  if (rc) return rc;
  rc = force_partials(w, ws, x, n, lx, r, m, lr, st);
  if (rc) return rc;
  return pair_force_reduce((const float*)((char*)ws + w.off_gpart), n, w.n_ch, s->dim, 1.0 / (double)m, force, st);
}

extern "C" int pdeinv_mf_mlp_step(const pdeinv_sde_desc* d, const pdeinv_mlp_shape* s, int32_t step, const float* z,
                                  float* z_out, float* tau_row, const float* ref, int64_t m, int64_t ldr, void* ws,
                                  void* stream) {
  PDEINV_REQUIRE(d != nullptr, PDEINV_ERR_INVALID, "mf_mlp_step: null descriptor");
  int rc = check_shape_ws(s, ws, false);
  if (rc) return rc;
  PDEINV_REQUIRE(d->potential.kind == PDEINV_POT_MEANFIELD_MLP, PDEINV_ERR_INVALID,
                 "mf_mlp_step: potential kind must be PDEINV_POT_MEANFIELD_MLP");
  PDEINV_REQUIRE(d->dim == s->dim, PDEINV_ERR_INVALID, "mf_mlp_step: descriptor and shape disagree on dim");
  SdeArgs sa;
  rc = build_args_without_potential(d, sa);
  if (rc) return rc;
  PDEINV_REQUIRE(step >= 0 && step <= d->n_steps, PDEINV_ERR_INVALID, "mf_mlp_step: s out of range");
  PDEINV_REQUIRE(d->d_shift_u == nullptr, PDEINV_ERR_INVALID,
                 "mf_mlp_step: the shared tau0 is drawn from the stream (shift_u unsupported)");
  PDEINV_REQUIRE(m >= 1, PDEINV_ERR_INVALID, "mf_mlp_step: m < 1 (the mean over an empty reference set)");
  const int64_t lr = ldr ? ldr : s->dim;
  PDEINV_REQUIRE(lr >= s->dim, PDEINV_ERR_INVALID, "mf_mlp_step: ldr < dim");
  if (sa.N == 0) return PDEINV_OK;
  PDEINV_REQUIRE(z != nullptr && z_out != nullptr && ref != nullptr, PDEINV_ERR_INVALID,
                 "mf_mlp_step: z / z_out / ref is null");
  PDEINV_REQUIRE(aligned(z, 4) && aligned(z_out, 4) && aligned(ref, 4) && aligned(tau_row, 4), PDEINV_ERR_INVALID,
                 "mf_mlp_step: pointers must be 4-byte aligned");
  rc = check_shape_ws(s, ws, true);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const Ws w = ws_plan(s, sa.N, m);
  rc = force_partials(w, ws, z, sa.N, sa.ld_z0, ref, m, lr, st);
  if (rc) return rc;
  StepArgs a{};
  a.N = sa.N; a.poff = sa.poff; a.ld_z = sa.ld_z0;
  a.s = step; a.n_steps = sa.n_steps; a.n_ch = w.n_ch;
  a.dt = sa.dt; a.gamma = sa.gamma; a.ns = sa.ns;
  a.tau0 = shared_tau0_host(sa, d);
  a.k0 = sa.k0; a.k1 = sa.k1; a.ctr_off = sa.ctr_off;
  a.noise = sa.noise;
  a.inv_m = 1.0 / (double)m;
  const float* gpart = (const float*)((char*)ws + w.off_gpart);
  const dim3 gr((unsigned)((sa.N + kBlock - 1) / kBlock)), bl(kBlock);
  switch (s->dim) {
#define CASE(DD)                                                                                      \
  case DD:                                                                                            \
    hipLaunchKernelGGL(mf_mlp_step_kernel<DD>, gr, bl, 0, st, a, gpart, z, z_out, tau_row);           \
    break;
    CASE(1) CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8)
#undef CASE
    default:
      return fail(PDEINV_ERR_UNSUPPORTED, kEnvelope);
  }
  return check_launch("mf_mlp_step_kernel");
}
