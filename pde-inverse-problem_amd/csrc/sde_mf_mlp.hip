// sde_mf_mlp.hip — the learned interaction Phi_theta = V_hypothesis (core/model.py:32-62) of the kinetic
// McKean–Vlasov system as a force and as the simulator's interaction (gfx950):
//   pdeinv_mf_mlp_force   F_i = (1/m) sum_{j<m} grad Phi_theta(x_i - r_j) for items x [n] against references r [m]
//                         (the pairwise mean of kinetic_mckean_vlasov.py:20-23, x_minus_ref; the self pair counts);
//   pdeinv_mf_mlp_step    one update of utils/sampling_utils.py:6-22 for this call's particles with that force,
//                         the references being the gathered positions of the whole ensemble (all ranks);
//   pdeinv_mf_mlp_prepare the weight image, once per simulate, into the workspace the steps read.
//
// Force kernel. The layout of pass 1 of the KMV residual (kmvq_gbar_kernel, mlp_pairs_mfma.hip) with separate item
// and reference sets: a wave owns one (item, chunk of kChunk references by reference index) unit, walks the chunk in
// 16-pair tiles — the pair on lane & 15, y = x_i - r_j formed in fp32 — and runs mlpq::tile_grad on each (every
// product a v_mfma_f32_16x16x4_f32, the weight image staged once per persistent block). The tile gradients of a lane
// add up in registers in tile order, the 16 lanes of a coordinate fold in a fixed butterfly, and the unit's D sums
// go to gpart[item][chunk]. No atomics. Tail tiles and the short last chunk load from a clamped row index (always
// inside r) and are masked after the load; their pairs run the tile at y = 0 and are dropped by a select.
// An item's numbers depend on its own row and on the reference set in its order only: the chunk grid is fixed by the
// reference index, not by n, by the items that share the call, or by the launch grid.
//
// Reduce / step. The chunk partials of an item are summed in chunk order in fp64 and scaled by 1/m (reduce_chunks:
// what kmvq_gbar_reduce_kernel does). The batch entry does that in a small kernel of its own; the simulator's step
// does it at the head of the update kernel instead of through a force array: the update is one thread per particle
// with 2d floats of state, so the fused form saves a launch and a round trip of [N, d] per update and costs nothing
// (n_ch <= 20 partials per coordinate at N = 5000). Both call the same function, so the step's force is the batch
// entry's bit for bit. The update itself is mf_step_kernel's (sde.hip): the Philox stream of include/pdeinv.h through
// stream_normals with the global id as the counter, explicit d_noise honoured, the shared clock tau0 of the
// ensemble (shared_tau0_host), h = tau0 / dt / dt - tau0.
#include <math.h>

#include "common.h"
#include "mlp_tile.h"
#include "sde_common.h"

namespace pdeinv {
namespace mlpmf {

using namespace mlpq;

constexpr int kWavesB = 8;  // waves per block: two blocks per CU = 4 waves per SIMD
constexpr int kThreads = kWavesB * kWave;
constexpr int kChunk = 256;  // references per work unit (16 tiles): pass 1's

struct ForceArgs {
  int64_t n, m, ldx, ldr, n_units;
  int32_t n_ch;
  const float* x;
  const float* r;
  float* gpart;  // [n][n_ch][D]
  TileNet net;
};

template <int KD>
__global__ __launch_bounds__(kThreads, 2) void mf_mlp_force_kernel(ForceArgs a) {
  extern __shared__ f32x4 lds4[];
  float* img = reinterpret_cast<float*>(lds4);
  for (int q = threadIdx.x; q < a.net.img_floats / 4; q += blockDim.x)
    lds4[q] = reinterpret_cast<const f32x4*>(a.net.img)[q];
  __syncthreads();
  const int lane0 = threadIdx.x & (kWave - 1), p = lane0 & 15, g = lane0 >> 4;
  const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int64_t wave = (int64_t)blockIdx.x * kWavesB + wib;
  const int64_t n_waves = (int64_t)gridDim.x * kWavesB;
  const int D = a.net.D;
  for (int64_t unit = wave; unit < a.n_units; unit += n_waves) {
    const int64_t it = unit / a.n_ch, ch = unit - it * a.n_ch;
    const int64_t j_end = (ch + 1) * kChunk < a.m ? (ch + 1) * kChunk : a.m;
    float xi[KD];
    lane_dims<KD>(a.x + it * a.ldx, D, g, xi);
    // reference row j of this lane's coordinates: an unconditional load from a clamped (row, coordinate), masked after
    auto load_ref = [&](int64_t j, float (&xn)[KD]) {
#pragma unroll
      for (int kk = 0; kk < KD; ++kk) {
        const int k = 4 * kk + g;
        const float v = a.r[(j < j_end ? j : j_end - 1) * a.ldr + (k < D ? k : D - 1)];
        xn[kk] = (j < j_end && k < D) ? v : 0.f;
      }
    };
    f32x4 gacc = {};
    float xn[KD];
    load_ref(ch * kChunk + p, xn);
    for (int64_t j0 = ch * kChunk; j0 < j_end; j0 += 16) {
      // the weight fragments are the same for every tile: an opaque lane index keeps the compiler from hoisting
      // all of them out of the tile loop (hundreds of VGPRs)
      int lane = lane0;
      asm volatile("" : "+v"(lane));
      const bool active = j0 + p < j_end;
      float yb[KD];
#pragma unroll
      for (int kk = 0; kk < KD; ++kk) yb[kk] = (active && 4 * kk + g < D) ? xi[kk] - xn[kk] : 0.f;
      load_ref(j0 + 16 + p, xn);  // the next tile's rows, under this tile's products
      float unused;
      const f32x4 ga = tile_grad<KD, false>(img, a.net, lane, yb, unused);
#pragma unroll
      for (int r = 0; r < 4; ++r) gacc[r] += active ? ga[r] : 0.f;
    }
    // sum over the 16 pairs of the lane row, coordinates 4 g + r
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float v = gacc[r];
#pragma unroll
      for (int off = 8; off > 0; off >>= 1) v += __shfl_xor(v, off, 16);
      const int k = 4 * g + r;
      if (p == 0 && k < D) a.gpart[unit * D + k] = v;
    }
  }
}

// coordinate k of item `it`: inv_m sum_ch gpart[it][ch][k], chunks in order, fp64
__device__ __forceinline__ float reduce_chunks(const float* __restrict__ gpart, int64_t it, int n_ch, int D, int k,
                                               double inv_m) {
  double s = 0.0;
  for (int c = 0; c < n_ch; ++c) s += (double)gpart[(it * n_ch + c) * D + k];
  return (float)(s * inv_m);
}

__global__ __launch_bounds__(kBlock) void mf_mlp_reduce_kernel(const float* __restrict__ gpart, int64_t n, int n_ch,
                                                               int D, double inv_m, float* __restrict__ force) {
  const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (q >= n * D) return;
  const int64_t it = q / D;
  force[q] = reduce_chunks(gpart, it, n_ch, D, (int)(q - it * D), inv_m);
}

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
static bool shape_ok(const pdeinv_mlp_shape* s) {
  return s->dim >= 1 && s->n_layers >= 1 && s->width >= 1 && s->out_features >= 1;
}
static bool tile_envelope(const pdeinv_mlp_shape* s) {
  return shape_ok(s) && s->dim <= 8 && s->width <= kW && s->n_layers <= kLMax;
}
static const char* const kEnvelope =
    "mf_mlp: the learned-interaction kernels cover dim <= 8, width <= 20, 1 <= n_layers <= 8";

static int device_cus() {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
    cus = 256;
  return cus;
}

// workspace: [image | h0y0 (W + O doubles) | gpart (n items x n_ch x D floats)], 256-byte pieces
struct Ws {
  ImagePlan ip;
  int n_ch;
  size_t off_img, off_h0, off_gpart, total, lds;
};
static Ws ws_plan(const pdeinv_mlp_shape* s, int64_t n, int64_t m) {
  Ws w{};
  w.ip = image_plan(s->dim, s->n_layers, s->width, s->out_features);
  w.n_ch = (int)((m + kChunk - 1) / kChunk);
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o += (bytes + 255) & ~(size_t)255; return at; };
  w.off_img = take(sizeof(float) * (size_t)w.ip.ia.img_floats);
  w.off_h0 = take(sizeof(double) * (size_t)(s->width + s->out_features));
  w.off_gpart = take(sizeof(float) * (size_t)n * (size_t)w.n_ch * (size_t)s->dim);
  w.total = o;
  w.lds = sizeof(float) * (size_t)w.ip.ia.img_floats;
  return w;
}

// the chunk partials of items x [n] against references r [m] into the workspace's gpart (the image is in place)
static int launch_force(const Ws& w, void* ws, const float* x, int64_t n, int64_t ldx, const float* r, int64_t m,
                        int64_t ldr, hipStream_t st) {
  ForceArgs a{};
  a.n = n; a.m = m; a.ldx = ldx; a.ldr = ldr;
  a.n_ch = w.n_ch;
  a.n_units = n * w.n_ch;
  a.x = x; a.r = r;
  a.gpart = (float*)((char*)ws + w.off_gpart);
  a.net = tile_net(w.ip, (const float*)((char*)ws + w.off_img));
  const int64_t need = (a.n_units + kWavesB - 1) / kWavesB, cap = 2 * (int64_t)device_cus();
  const dim3 gr((unsigned)(need < cap ? need : cap)), bl(kThreads);
  if (w.ip.KD == 1) {
    (void)hipFuncSetAttribute((const void*)mf_mlp_force_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              160 * 1024);
    hipLaunchKernelGGL(mf_mlp_force_kernel<1>, gr, bl, w.lds, st, a);
  } else {
    (void)hipFuncSetAttribute((const void*)mf_mlp_force_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              160 * 1024);
    hipLaunchKernelGGL(mf_mlp_force_kernel<2>, gr, bl, w.lds, st, a);
  }
  return check_launch("mf_mlp_force_kernel");
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
  PDEINV_REQUIRE(shape_ok(s), PDEINV_ERR_INVALID, "mf_mlp: dim, n_layers, width and out_features must be >= 1");
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
  const Ws w = ws_plan(s, 0, 1);  // the image and h0y0 offsets do not depend on n, m
  return build_image(w.ip.ia, params, (double*)((char*)ws + w.off_h0), (float*)((char*)ws + w.off_img),
                     (hipStream_t)stream);
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
  rc = build_image(w.ip.ia, params, (double*)((char*)ws + w.off_h0), (float*)((char*)ws + w.off_img), st);
  if (rc) return rc;
  rc = launch_force(w, ws, x, n, lx, r, m, lr, st);
  if (rc) return rc;
  const int64_t nq = n * s->dim;
  hipLaunchKernelGGL(mf_mlp_reduce_kernel, dim3((unsigned)((nq + kBlock - 1) / kBlock)), dim3(kBlock), 0, st,
                     (const float*)((char*)ws + w.off_gpart), n, w.n_ch, (int)s->dim, 1.0 / (double)m, force);
  return check_launch("mf_mlp_reduce_kernel");
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
  pdeinv_sde_desc dd = *d;  // the shared descriptor checks; the potential's fields are not read
  dd.potential = pdeinv_potential{};
  dd.potential.kind = PDEINV_POT_NONE;
  SdeArgs sa;
  rc = build_args(&dd, sa);
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
  rc = launch_force(w, ws, z, sa.N, sa.ld_z0, ref, m, lr, st);
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
