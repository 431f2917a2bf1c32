// realnvp.hip — the time-conditioned RealNVP flow (core/normalizing_flow.py:8-229) in five parts:
//  1. realnvp_logdensity_kernel: log p_t(x), one thread per (t, x) sample, the tiny MLPs (widths 8 / 16 / 16,
//     SURVEY.md §8(a) a12) in VGPRs on the VALU, weights at wave-uniform addresses (scalar loads). Helpers:
//     nvp_act, dense, basic_mlp.
//  2. realnvp_grad_kernel (+ nvp_slab_split_kernel, nvp_grad_reduce_kernel): value and parameter gradient of the
//     maximum-likelihood loss on the matrix cores, 16-sample tiles. Helpers: the tile machinery nv_* (NvM / NvC /
//     NvScr layouts, NvLane, nv_fwdT, nv_wgrad, nv_mlp_fwd / _bwd, nv_put_*, nv_layer_dst, nv_slab_col).
//  3. The time derivatives (log p, d/dt, d2/dt2): realnvp_time_kernel (general, one thread per sample; helpers
//     nvp_act_d2, nvp_act3, dense3_*, basic_mlp3) and realnvp_time_mfma_kernel (matrix cores; nv_fwdT3, nv_bias3,
//     nv_celu3, nv_mlp_fwd3 on part 2's tile machinery).
//  4. The flow as a map in either direction (y, ldj, log p; pdeinv_realnvp_map): realnvp_map_kernel (general, one
//     thread per sample, part 1's arithmetic over a compile-time direction) and realnvp_map_mfma_kernel (matrix
//     cores: part 2's likelihood pass on its tile machinery, run forwards or backwards through the layers).
//  5. The score grad_x log p (pdeinv_realnvp_score), reverse mode with each layer's input kept in a workspace:
//     realnvp_score_kernel (general, one thread per sample; helpers nvp_dense_d1, nvp_mlp_d1, nvp_mlp_bwd_x on part
//     3's nvp_act_d2) and realnvp_score_mfma_kernel (matrix cores: part 2's likelihood pass and backward sweep without
//     its weight gradients; helper nv_mlp_bwd_in); nvp_couple1 is the coupling update of both, in both passes.
// Shared: NvpArgs (masks and the base Gaussian travel in the kernel arguments) and nvp_temb_params by all;
// the block-level staging nv_lane / nv_stage_* by the four tile kernels; nv_prefetch, nv_masked and nv_group_sum by
// the gradient, map and score tile kernels, nv_scatter_layer by the gradient and map tile kernels (see "blocks of the
// tile kernels' bodies"); the three-stream arithmetic nvp_act3, NVP_COUPLE3 and NVP_BASE_STORE3 (macros: see there)
// by the two time kernels; on the host one descriptor check (NVP_REQUIRE_DESC), one NvpArgs fill (nvp_args), one
// path choice (NVP_IMPL_PATH over nvp_tile_ok) for the map and the score, and one (dim, activation) launch table
// (NVP_LAUNCH_DIM_ACT) for the general time and score kernels.
// Still written out in each kernel, because compiled from one shared definition the kernel's register, spill or LDS
// figures move (DESIGN.md §13.2 has each figure): in the tile kernels the staging of a layer around nv_scatter_layer
// (the score kernel's scatter too), the tile load, the time embedding's forward (in realnvp_grad_kernel also a
// second time for the backward: see the comment there), the base form from a __shfl gather, the owning-lane row
// store, and realnvp_time_mfma_kernel's sum over the lane groups; in the general path the time embedding and the
// coupling update of realnvp_logdensity_kernel and realnvp_map_kernel, and the former's base form. Also the three
// lines of sample addressing (per-sample / sets view) in the two time kernels.
#include <math.h>

#include "common.h"

namespace pdeinv {

struct NvpArgs {
  int n_layers, E, in_dim, ignore_time, act;
  float soft_init, log_det;
  float mean[8], inv_cov[64];
  float masks[PDEINV_REALNVP_MAX_LAYERS * 8];
};

// Parameters of the time embedding (two E x E dense layers), in front of the coupling layers; none for E = 0.
__host__ __device__ constexpr int64_t nvp_temb_params(int E) { return E > 0 ? 2 * ((int64_t)E * E + E) : 0; }

__device__ __forceinline__ float nvp_act(int act, float x) {
  switch (act) {
    case PDEINV_ACT_CELU: return x > 0.f ? x : expm1f(x);  // jax.nn.celu, alpha = 1
    case PDEINV_ACT_RELU: return fmaxf(x, 0.f);
    case PDEINV_ACT_TANH: return tanhf(x);
    case PDEINV_ACT_ELU: return x > 0.f ? x : expm1f(x);
    case PDEINV_ACT_SILU: return x / (1.f + expf(-x));
    case PDEINV_ACT_SOFTPLUS: return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x)));
    default: {  // gelu, tanh approximation
      const float c = 0.7978845608028654f;  // sqrt(2 / pi)
      return 0.5f * x * (1.f + tanhf(c * (x + 0.044715f * x * x * x)));
    }
  }
}

// y[out] = act?(b + in @ W), W [n_in x n_out] row-major at p, b right after it.
template <int NI, int NO>
__device__ __forceinline__ const float* dense(const float* __restrict__ p, const float (&in)[NI], int n_in,
                                              float (&out)[NO], int act, bool apply_act) {
  const float* b = p + n_in * NO;
#pragma unroll
  for (int o = 0; o < NO; ++o) out[o] = b[o];
  for (int i = 0; i < n_in; ++i) {
    const float v = in[i];
#pragma unroll
    for (int o = 0; o < NO; ++o) out[o] = fmaf(v, p[i * NO + o], out[o]);
  }
  if (apply_act) {
#pragma unroll
    for (int o = 0; o < NO; ++o) out[o] = nvp_act(act, out[o]);
  }
  return b + NO;
}

template <int D>
__device__ __forceinline__ const float* basic_mlp(const float* p, const float (&in)[D + 16], int n_in, int act,
                                                  float (&out)[D]) {
  float h0[8], h1[16], h2[16];
  p = dense<D + 16, 8>(p, in, n_in, h0, act, true);
  p = dense<8, 16>(p, h0, 8, h1, act, true);
  p = dense<16, 16>(p, h1, 16, h2, act, true);
  return dense<16, D>(p, h2, 16, out, act, false);
}

template <int D>
__global__ __launch_bounds__(kBlock) void realnvp_logdensity_kernel(NvpArgs a, const float* __restrict__ params,
                                                                    const float* __restrict__ tv, int64_t t_stride,
                                                                    const float* __restrict__ xv, int64_t n,
                                                                    int64_t ld, int64_t layer_stride,
                                                                    float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const float t = tv[i * t_stride];
  float x[D];
#pragma unroll
  for (int k = 0; k < D; ++k) x[k] = xv[i * ld + k];
  // time embedding (shared by every coupling layer)
  float temb[16];
  const float* p = params;
  if (!a.ignore_time) {
    if (a.E > 0) {
      const int half = a.E / 2;
      const float step = logf(10000.f) / (float)(half - 1);
      float se[16], h[16];
      for (int k = 0; k < half; ++k) {
        const float e = t * expf(-step * (float)k);
        se[k] = sinf(e);
        se[half + k] = cosf(e);
      }
      // two E x E dense layers (runtime E <= 16)
      for (int o = 0; o < a.E; ++o) h[o] = p[a.E * a.E + o];
      for (int q = 0; q < a.E; ++q)
        for (int o = 0; o < a.E; ++o) h[o] = fmaf(se[q], p[q * a.E + o], h[o]);
      for (int o = 0; o < a.E; ++o) h[o] = nvp_act(a.act, h[o]);
      p += a.E * a.E + a.E;
      for (int o = 0; o < a.E; ++o) temb[o] = p[a.E * a.E + o];
      for (int q = 0; q < a.E; ++q)
        for (int o = 0; o < a.E; ++o) temb[o] = fmaf(h[q], p[q * a.E + o], temb[o]);
      p += a.E * a.E + a.E;
    } else {
      temb[0] = t;
    }
  }
  const float* layers = p;
  float ldj = 0.f;
  for (int l = a.n_layers - 1; l >= 0; --l) {  // likelihood direction: reversed layers
    const float* lp = layers + (int64_t)l * layer_stride;
    const float* m = a.masks + l * D;
    float in[D + 16];
#pragma unroll
    for (int k = 0; k < D; ++k) in[k] = x[k] * m[k];
    const int n_t = a.in_dim - D;
    for (int q = 0; q < n_t; ++q) in[D + q] = temb[q];
    float s[D], tr[D];
    const float* sfp = lp;
    const float* q = basic_mlp<D>(lp + D, in, a.in_dim, a.act, s);
    basic_mlp<D>(q, in, a.in_dim, a.act, tr);
    const bool hard = !a.ignore_time && a.soft_init == 0.f;
#pragma unroll
    for (int k = 0; k < D; ++k) {
      float sk = hard ? t * s[k] : s[k];
      float tk = hard ? t * tr[k] : tr[k];
      const float sf = expf(sfp[k]);
      sk = tanhf(sk / sf) * sf;
      sk *= 1.f - m[k];
      tk *= 1.f - m[k];
      x[k] = (x[k] + tk) * expf(sk);
      ldj += sk;
    }
  }
  float quad = 0.f;
#pragma unroll
  for (int r = 0; r < D; ++r) {
    float acc = 0.f;
#pragma unroll
    for (int c = 0; c < D; ++c) acc = fmaf(a.inv_cov[r * D + c], x[c] - a.mean[c], acc);
    quad = fmaf(x[r] - a.mean[r], acc, quad);
  }
  out[i] = -0.5f * (a.log_det + quad) + ldj;
}

// (x - mean)^T inv_cov (x - mean) of the base Gaussian
template <int D>
__device__ __forceinline__ float nvp_base_quad(const NvpArgs& a, const float (&x)[D]) {
  float quad = 0.f;
#pragma unroll
  for (int r = 0; r < D; ++r) {
    float acc = 0.f;
#pragma unroll
    for (int c = 0; c < D; ++c) acc = fmaf(a.inv_cov[r * D + c], x[c] - a.mean[c], acc);
    quad = fmaf(x[r] - a.mean[r], acc, quad);
  }
  return quad;
}

// The flow as a map, one kernel body over the direction (pdeinv_realnvp_map's general path), with the arithmetic
// of realnvp_logdensity_kernel statement for statement: <D, 1>'s out is that kernel's, bit for bit. (That kernel is
// not this body's (REV = 1, no y) case: compiled from this body it moves a 16-float array into LDS, 16 KB per block.
// The same happens to it with nvp_base_quad in place of its own loop, and a shared time embedding or coupling update
// moves the register and spill figures of both kernels: DESIGN.md §13.2.)
//   REV = 1: layers L-1 .. 0, x <- (x + tr) e^s,  ldj += sum s, out = log p0(y) + ldj    (likelihood direction)
//   REV = 0: layers 0 .. L-1, x <- x e^{-s} - tr, ldj -= sum s, out = log p0(x_in) - ldj (generation)
// y (row stride ld_y), ldj_out and out are each nullable. y may be xv itself (in place: a thread has read its row
// before it writes it), so neither pointer is restrict.
template <int D, int REV>
__global__ __launch_bounds__(kBlock) void realnvp_map_kernel(NvpArgs a, const float* __restrict__ params,
                                                                    const float* __restrict__ tv, int64_t t_stride,
                                                                    const float* xv, int64_t n, int64_t ld,
                                                                    int64_t layer_stride, float* y, int64_t ld_y,
                                                                    float* __restrict__ ldj_out,
                                                                    float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const float t = tv[i * t_stride];
  float x[D];
#pragma unroll
  for (int k = 0; k < D; ++k) x[k] = xv[i * ld + k];
  float quad = 0.f;  // the base quadratic form of the point in latent space: the input (REV = 0) or the output
  if (!REV && out) quad = nvp_base_quad<D>(a, x);
  // time embedding (shared by every coupling layer)
  float temb[16];
  const float* p = params;
  if (!a.ignore_time) {
    if (a.E > 0) {
      const int half = a.E / 2;
      const float step = logf(10000.f) / (float)(half - 1);
      float se[16], h[16];
      for (int k = 0; k < half; ++k) {
        const float e = t * expf(-step * (float)k);
        se[k] = sinf(e);
        se[half + k] = cosf(e);
      }
      // two E x E dense layers (runtime E <= 16)
      for (int o = 0; o < a.E; ++o) h[o] = p[a.E * a.E + o];
      for (int q = 0; q < a.E; ++q)
        for (int o = 0; o < a.E; ++o) h[o] = fmaf(se[q], p[q * a.E + o], h[o]);
      for (int o = 0; o < a.E; ++o) h[o] = nvp_act(a.act, h[o]);
      p += a.E * a.E + a.E;
      for (int o = 0; o < a.E; ++o) temb[o] = p[a.E * a.E + o];
      for (int q = 0; q < a.E; ++q)
        for (int o = 0; o < a.E; ++o) temb[o] = fmaf(h[q], p[q * a.E + o], temb[o]);
      p += a.E * a.E + a.E;
    } else {
      temb[0] = t;
    }
  }
  const float* layers = p;
  float ldj = 0.f;
  for (int j = 0; j < a.n_layers; ++j) {
    const int l = REV ? a.n_layers - 1 - j : j;  // likelihood direction: reversed layers
    const float* lp = layers + (int64_t)l * layer_stride;
    const float* m = a.masks + l * D;
    float in[D + 16];
#pragma unroll
    for (int k = 0; k < D; ++k) in[k] = x[k] * m[k];
    const int n_t = a.in_dim - D;
    for (int q = 0; q < n_t; ++q) in[D + q] = temb[q];
    float s[D], tr[D];
    const float* sfp = lp;
    const float* q = basic_mlp<D>(lp + D, in, a.in_dim, a.act, s);
    basic_mlp<D>(q, in, a.in_dim, a.act, tr);
    const bool hard = !a.ignore_time && a.soft_init == 0.f;
#pragma unroll
    for (int k = 0; k < D; ++k) {
      float sk = hard ? t * s[k] : s[k];
      float tk = hard ? t * tr[k] : tr[k];
      const float sf = expf(sfp[k]);
      sk = tanhf(sk / sf) * sf;
      sk *= 1.f - m[k];
      tk *= 1.f - m[k];
      if (REV) {
        x[k] = (x[k] + tk) * expf(sk);
        ldj += sk;
      } else {
        x[k] = x[k] * expf(-sk) - tk;
        ldj -= sk;
      }
    }
  }
  if (y) {
#pragma unroll
    for (int k = 0; k < D; ++k) y[i * ld_y + k] = x[k];
  }
  if (ldj_out) ldj_out[i] = ldj;
  if (REV) {
    if (out) {
      quad = nvp_base_quad<D>(a, x);
      out[i] = -0.5f * (a.log_det + quad) + ldj;
    }
  } else if (out) {
    out[i] = -0.5f * (a.log_det + quad) - ldj;
  }
}


// ---------------------------------------------------------------------------------------------
// Value and parameter gradient of the maximum-likelihood loss (log_density_estimation.py:47-58):
// loss = -mean_i log p_{t_i}(x_i), replacing jax.value_and_grad(loss_fn).
//
// Matrix-core formulation (v_mfma_f32_16x16x4_f32, exact fp32). Samples go in tiles of 16; every
// per-sample 16-vector (x, its gradient, the time embedding, each hidden layer) lives in the
// MFMA accumulator layout: lane (g = lane / 16, s = lane % 16) holds components 4g .. 4g + 3 of
// sample s. A dense layer out = W^T in is four MFMAs whose B operand at k-step j is register j of
// that same layout — k-slot (j, g) stands for input component 4g + j, and the A operand (the
// weights, read from LDS) is permuted to match — so layers chain with no data movement at all.
// The input-gradient product W d uses the transposed read of the same LDS matrix. Weight
// gradients sum_s a_s d_s^T take the samples as the reduction dimension: each tile goes through a
// per-wave swizzled LDS stage (one 16-byte write per lane, one read per k-step) into four MFMAs
// whose accumulators (ΔW in the same layout, rows = inputs) stay in registers over the wave's
// tiles. Bias and scaling-factor gradients are per-lane sums, summed over the samples at the flush
// (a reduce-scatter butterfly for a net's four bias vectors).
// All widths are padded to 16 (the net's first layer: 8 outputs; x: d <= 8 coordinates; time:
// n_t <= 16 features) with zero weights, so padded components stay exactly 0.
// * The backward pass walks the coupling layers in the opposite order of the likelihood pass and
//   rebuilds each layer's input by inverting the layer (x_in = x_out e^{-s} - tr; the masked
//   coordinates, which feed s and tr, pass through unchanged and exact): no per-layer state.
// * Per coupling layer the block sums its four waves' compact partial blocks (NvC) as float4 into its
//   slab row; the split reduce reads slab column nv_slab_col(c) for reference parameter c (the loss
//   after the time embedding's columns), and a fixed-order fp64 column reduce gives grad = -1/n sum.
//   No float atomics: bit-reproducible run to run.
// * Packed layout (d <= 4, time features <= 12): 49 KB of LDS per block and 168 VGPRs, three waves per
//   SIMD.
// Built for the celu / elu activation (the flow of log_density_estimation.py:103-114).
// ---------------------------------------------------------------------------------------------
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kNvpMaxRows = 8192;  // slab rows (128-sample blocks) per launch + reduce chunk
constexpr int kNvT = 2;            // 16-sample tiles per wave (32 samples; 128 per block)
constexpr int kNvWavesPk = 3;      // waves per SIMD of the packed-layout gradient kernel (49 KB LDS per block)
constexpr int kNvWaves = 2;        // waves per SIMD of the identity-layout gradient kernel
constexpr int kNvSPB = kWavesPerBlock * 16 * kNvT;  // samples per block = per slab row
constexpr int kNvWS = 20;          // LDS row stride of a padded 16 x 16 weight matrix
// Per-wave sample stage: [16 samples][16 components] dense, the 4-float chunk c of sample row r stored at chunk
// c ^ nv_swz(r). Its 16-byte writes (8-lane groups, rows s = 0..7 of one chunk) and its 4-byte reads (32-lane
// groups, rows 4t + {0, 1}, 16 components each) then cover the 32 banks of each lane group exactly once.
constexpr int kNvSS = 16;
__device__ __forceinline__ int nv_swz(int r) { return (r >> 1) & 3; }
constexpr int kNvRaw = 8 + 2 * (24 * 8 + 8 + 128 + 16 + 256 + 16 + 16 * 8 + 8);  // one layer's params, d <= 8
constexpr int kNvPre = (kNvRaw + kBlock - 1) / kBlock;

// Activation derivative from the post-activation value h (celu / elu: e^z = h + 1): min(h + 1, 1).
__device__ __forceinline__ float nvp_celu_grad_h(float h) { return fminf(h + 1.f, 1.f); }
// hardware exp2 / rcp (v_exp_f32, v_rcp_f32: ~1 ulp; the grad kernel's transcendentals)
__device__ __forceinline__ float nv_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.4426950408889634f); }
__device__ __forceinline__ float nv_tanh(float x) { return 1.f - 2.f * __builtin_amdgcn_rcpf(nv_exp(2.f * x) + 1.f); }
// celu(z) = median(z, e^z - 1, 0): e^z - 1 >= z everywhere, so the median is z for z > 0 and e^z - 1 for
// z <= 0 (one v_med3 instead of a compare and a select).
__device__ __forceinline__ float nvp_celu(float z) { return __builtin_amdgcn_fmed3f(z, nv_exp(z) - 1.f, 0.f); }

// Padded LDS layout of one BasicMLP (weights [in][out] with row stride kNvWS), one coupling layer
// and the time embedding.
// Each matrix is also stored transposed (suffix T): the input-gradient product W d then reads it with
// the same bank-conflict-free pattern as the forward (a transposed read of W itself is 4-way).
// Packed layout: no W0X (the joined first layer is W0T). The layer image carries the layer's mask (by
// position, padded with 1) after sf. The time embedding's matrices use the same LDS array before the first
// and after the last coupling layer (TEMB floats at its start).
template <bool PK>
struct NvM {
  static constexpr int MAT = 16 * kNvWS;
  static constexpr int W0T = 0, W0X = PK ? 0 : MAT, W1 = W0X + MAT, W2 = W1 + MAT, W3 = W2 + MAT,
                       TR = W3 + MAT,  // W^T at +TR
                       B0 = 2 * TR, B1 = B0 + 16, B2 = B1 + 16, B3 = B2 + 16, NET = B3 + 16;
  static constexpr int SF = 0, MASK = 16, SNET = 32, TNET = 32 + NET, LAYER = 32 + 2 * NET;
  static constexpr int E_W1 = 0, E_B1 = MAT, E_W2 = MAT + 16, E_B2 = 2 * MAT + 16, E_W2T = 2 * MAT + 32,
                       TEMB = 3 * MAT + 32;
  static_assert(TEMB <= LAYER, "time embedding inside the layer image");
};
// Per-wave partial-gradient block of one coupling layer, compact (only the entries a parameter maps to):
// [t-net | s-net | sf (16, by position)]. Per net, packed layout: W0 [16 input positions][8 hidden units],
// W1 [8][16], W2 [16][16], W3 [16][4 coordinates], b0..b3 by position (16 each); identity layout: W0T
// [16 time rows][8], W0X [8 coordinates][8], W1 [8][16], W2, W3 [16][8], b0..b3. The block is also the layer's
// slab-row segment (the flush sums the four waves' blocks as float4 into it); the reduce maps it to the
// reference parameter order (nv_slab_col). In LDS the t-net part aliases the wave's sample stage (it is written
// after the t-net's last weight gradient) and the s-net part + sf sit behind the stage (written as soon as the
// s-net's backward is done, so its accumulators are dead during the t-net's). The time embedding's flush reuses
// the first 2 x 272 floats.
template <bool PK>
struct NvC {
  static constexpr int W0T = 0, W0X = 128, W1 = PK ? 128 : 192, W2 = W1 + 128, W3 = W2 + 256,
                       B0 = W3 + (PK ? 64 : 128), B1 = B0 + 16, B2 = B1 + 16, B3 = B2 + 16, NET = B3 + 16;
  static constexpr int TNET = 0, SNET = NET, SF = 2 * NET, LAYER = 2 * NET + 16;  // 1296 / 1552 floats
};
constexpr int kNvStageF = 2 * 16 * kNvSS;  // per-wave sample stage (floats): one tile's two operands
// Per-wave scratch: [t-net block / sample stage (kNvTR floats) | s-net block | sf]
template <bool PK>
struct NvScr {
  static constexpr int TR = NvC<PK>::NET > kNvStageF ? NvC<PK>::NET : kNvStageF;
  static constexpr int SIZE = TR + NvC<PK>::NET + 16;
};
// LDS offset (in the wave's scratch) of compact-block entry o
template <bool PK>
__device__ __forceinline__ int nv_flush_lds(int o) { return o < NvC<PK>::NET ? o : o - NvC<PK>::NET + NvScr<PK>::TR; }

struct NvLane {
  int g, s;    // component group, sample within the tile
  int sw, sr;  // sample-stage offsets: this lane's 16-byte write (row s, chunk g); its read of row g, component s
};

// Position of a component in the padded 16-vectors. Packed layout (PK: d <= 4, n_t <= 12): coordinate c
// at 4c (register 0 of lane group c), time-embedding component e at 4(e / 3) + 1 + e % 3 (registers 1..3),
// the first hidden layer's 8 units at 4(o / 2) + o % 2 (registers 0, 1). So [x | temb] is ONE 16-vector
// with no data movement (register 0 from x, 1..3 from temb: the net's first layer is one 16 x 16 product,
// not two), and the k-steps whose inputs are all padding are skipped: W1 reads 2 of 4, the input-gradient
// products of W3 and W0 1 and 2 of 4. The matrices are permuted to match when a layer is staged (a
// dense layer's output order is the A operand's row order, free to choose). Identity layout otherwise.
template <bool PK> __device__ __forceinline__ int nv_xpos(int c) { return PK ? 4 * c : c; }
template <bool PK> __device__ __forceinline__ int nv_tpos(int e) { return PK ? 4 * (e / 3) + 1 + e % 3 : e; }
template <bool PK> __device__ __forceinline__ int nv_hpos(int o) { return PK ? 4 * (o / 2) + o % 2 : o; }
// inverses: position -> component, or -1 (padding); n = the component count
template <bool PK> __device__ __forceinline__ int nv_xinv(int p, int n) {
  const int c = PK ? ((p & 3) == 0 ? p >> 2 : -1) : p;
  return c < n ? c : -1;
}
template <bool PK> __device__ __forceinline__ int nv_tinv(int p, int n) {
  const int e = PK ? ((p & 3) != 0 ? 3 * (p >> 2) + (p & 3) - 1 : -1) : p;
  return e < n ? e : -1;
}
template <bool PK> __device__ __forceinline__ int nv_hinv(int p) {
  const int o = PK ? ((p & 3) < 2 ? 2 * (p >> 2) + (p & 3) : -1) : p;
  return o < 8 ? o : -1;
}

__device__ __forceinline__ f32x4 nv_vec(const float* b, const NvLane& ln) {
  return *reinterpret_cast<const f32x4*>(b + 4 * ln.g);
}
__device__ __forceinline__ f32x4 nv_celu4(f32x4 z) {
  return f32x4{nvp_celu(z[0]), nvp_celu(z[1]), nvp_celu(z[2]), nvp_celu(z[3])};
}
__device__ __forceinline__ f32x4 nv_dact4(f32x4 d, f32x4 h) {
  return f32x4{d[0] * nvp_celu_grad_h(h[0]), d[1] * nvp_celu_grad_h(h[1]), d[2] * nvp_celu_grad_h(h[2]),
               d[3] * nvp_celu_grad_h(h[3])};
}
// Order the wave's own LDS stage accesses (a wave's LDS instructions execute in order, so a lane
// reads what another lane of the same wave wrote before it) without fencing the MFMA / VALU
// stream: a compiler memory barrier only, so independent matrix work still moves across it.
__device__ __forceinline__ void nv_wave_sync() { asm volatile("" ::: "memory"); }
// The wave's kNvT tiles go through every dense layer together: one A-operand (weight) read feeds
// kNvT independent MFMAs, so the accumulation chains of the tiles interleave.
typedef f32x4 NvV[kNvT];

// k-steps j with JM bit j clear carry only padding inputs (all zero) and are skipped.
template <int JM = 0xF>
__device__ __forceinline__ void nv_fwdT(const float* W, const NvLane& ln, const NvV& x, NvV& c) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (!((JM >> j) & 1)) continue;
    const float av = W[(4 * ln.g + j) * kNvWS + ln.s];
#pragma unroll
    for (int u = 0; u < kNvT; ++u) c[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, x[u][j], c[u], 0, 0, 0);
  }
}
__device__ __forceinline__ void nv_bcast(NvV& c, const f32x4& b) {
#pragma unroll
  for (int u = 0; u < kNvT; ++u) c[u] = b;
}

// acc += sum over the wave's samples of a_s d_s^T (rows = a components): per-wave LDS stage
// [2][16 samples][kNvSS] (swizzled chunks, nv_swz) holding one tile at a time (a wave's LDS instructions run
// in order, so the next tile's writes follow this tile's reads): one 16-byte write per lane and operand, one
// read per operand and k-step.
__device__ __forceinline__ f32x4 nv_wgrad(float* stage, const NvLane& ln, const NvV& a, const NvV& d, f32x4 acc) {
#pragma unroll
  for (int u = 0; u < kNvT; ++u) {
    nv_wave_sync();  // the previous reads of the stage are issued
    *reinterpret_cast<f32x4*>(stage + ln.sw) = a[u];
    *reinterpret_cast<f32x4*>(stage + 16 * kNvSS + ln.sw) = d[u];
    nv_wave_sync();
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      // row 4t + g: nv_swz(4t + g) = nv_swz(g) ^ 2 (t & 1), i.e. component s ^ 8 on odd t
      const int r = 4 * t * kNvSS + (ln.sr ^ (t & 1 ? 8 : 0));
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(stage[r], stage[16 * kNvSS + r], acc, 0, 0, 0);
    }
  }
  return acc;
}

// Gradient accumulators of one BasicMLP over the wave's tiles.
struct NvNetAcc {
  f32x4 w0t, w0x, w1, w2, w3, b0, b1, b2, b3;
  __device__ void zero() { w0t = w0x = w1 = w2 = w3 = b0 = b1 = b2 = b3 = f32x4{0.f, 0.f, 0.f, 0.f}; }
};

struct NvAct {
  NvV h0, h1, h2;
};

// Packed layout: the net input [xm | temb] as one vector (register 0 from xm, 1..3 from temb).
__device__ __forceinline__ void nv_join(const NvV& xm, const NvV& temb, NvV& in) {
#pragma unroll
  for (int u = 0; u < kNvT; ++u) in[u] = f32x4{xm[u][0], temb[u][1], temb[u][2], temb[u][3]};
}

// BasicMLP (:97-111) forward: input [temb | xm], hidden 8 / 16 / 16, output d (all padded to 16).
// Packed layout: the first layer is one product over the joined input, stored at W0T.
template <bool PK>
__device__ __forceinline__ void nv_mlp_fwd(const float* p, const NvLane& ln, const NvV& temb, const NvV& xm,
                                           NvAct& h, NvV& out) {
  NvV z;
  nv_bcast(z, nv_vec(p + NvM<PK>::B0, ln));
  if constexpr (PK) {
    NvV in;
    nv_join(xm, temb, in);
    nv_fwdT(p + NvM<PK>::W0T, ln, in, z);
  } else {
    nv_fwdT(p + NvM<PK>::W0T, ln, temb, z);
    nv_fwdT(p + NvM<PK>::W0X, ln, xm, z);
  }
#pragma unroll
  for (int u = 0; u < kNvT; ++u) {
    if constexpr (PK)  // registers 2, 3: padding units (zero weights and bias), celu(0) = 0
      h.h0[u] = f32x4{nvp_celu(z[u][0]), nvp_celu(z[u][1]), 0.f, 0.f};
    else
      h.h0[u] = nv_celu4(z[u]);
  }
  nv_bcast(z, nv_vec(p + NvM<PK>::B1, ln));
  nv_fwdT<PK ? 0x3 : 0xF>(p + NvM<PK>::W1, ln, h.h0, z);
#pragma unroll
  for (int u = 0; u < kNvT; ++u) h.h1[u] = nv_celu4(z[u]);
  nv_bcast(z, nv_vec(p + NvM<PK>::B2, ln));
  nv_fwdT(p + NvM<PK>::W2, ln, h.h1, z);
#pragma unroll
  for (int u = 0; u < kNvT; ++u) h.h2[u] = nv_celu4(z[u]);
  nv_bcast(out, nv_vec(p + NvM<PK>::B3, ln));
  nv_fwdT(p + NvM<PK>::W3, ln, h.h2, out);
}

// BasicMLP backward from d(out): parameter gradients into acc, input gradients added to gtemb
// (time rows) and gx (x rows). The input-gradient products W d read the transposed copies.
// Packed layout: acc.w0t holds the joined first-layer gradient (acc.w0x unused).
template <bool PK>
__device__ __forceinline__ void nv_mlp_bwd(const float* p, const NvLane& ln, float* stage, const NvV& temb,
                                           const NvV& xm, const NvAct& h, const NvV& dout, NvNetAcc& acc,
                                           NvV& gtemb, NvV& gx) {
  const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
  NvV d, e;
  acc.w3 = nv_wgrad(stage, ln, h.h2, dout, acc.w3);
  nv_bcast(e, z4);
  nv_fwdT<PK ? 0x1 : 0xF>(p + NvM<PK>::TR + NvM<PK>::W3, ln, dout, e);
#pragma unroll
  for (int u = 0; u < kNvT; ++u) {
    acc.b3 += dout[u];
    d[u] = nv_dact4(e[u], h.h2[u]);
  }
  acc.w2 = nv_wgrad(stage, ln, h.h1, d, acc.w2);
  nv_bcast(e, z4);
  nv_fwdT(p + NvM<PK>::TR + NvM<PK>::W2, ln, d, e);
#pragma unroll
  for (int u = 0; u < kNvT; ++u) {
    acc.b2 += d[u];
    d[u] = nv_dact4(e[u], h.h1[u]);
  }
  acc.w1 = nv_wgrad(stage, ln, h.h0, d, acc.w1);
  nv_bcast(e, z4);
  nv_fwdT(p + NvM<PK>::TR + NvM<PK>::W1, ln, d, e);
#pragma unroll
  for (int u = 0; u < kNvT; ++u) {
    acc.b1 += d[u];
    if constexpr (PK)  // padding units: their gradient feeds only padding entries (dropped by the flush)
      d[u] = f32x4{e[u][0] * nvp_celu_grad_h(h.h0[u][0]), e[u][1] * nvp_celu_grad_h(h.h0[u][1]), 0.f, 0.f};
    else
      d[u] = nv_dact4(e[u], h.h0[u]);
  }
  if constexpr (PK) {
    NvV in;
    nv_join(xm, temb, in);
    acc.w0t = nv_wgrad(stage, ln, in, d, acc.w0t);
#pragma unroll
    for (int u = 0; u < kNvT; ++u) acc.b0 += d[u];
    nv_bcast(e, z4);
    nv_fwdT<0x3>(p + NvM<PK>::TR + NvM<PK>::W0T, ln, d, e);
#pragma unroll
    for (int u = 0; u < kNvT; ++u) {
      gx[u][0] += e[u][0];
#pragma unroll
      for (int c = 1; c < 4; ++c) gtemb[u][c] += e[u][c];
    }
  } else {
    acc.w0t = nv_wgrad(stage, ln, temb, d, acc.w0t);
    acc.w0x = nv_wgrad(stage, ln, xm, d, acc.w0x);
#pragma unroll
    for (int u = 0; u < kNvT; ++u) acc.b0 += d[u];
    nv_fwdT(p + NvM<PK>::TR + NvM<PK>::W0T, ln, d, gtemb);
    nv_fwdT(p + NvM<PK>::TR + NvM<PK>::W0X, ln, d, gx);
  }
}

// Sum of v over the 16 samples of each component group: DPP inside 16-lane rows (quad_perm xor 1,
// xor 2, row_half_mirror, row_mirror), every lane of the row ends with the row total.
template <int CTRL>
__device__ __forceinline__ float nv_dpp(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
__device__ __forceinline__ f32x4 nv_sum16(f32x4 v) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[i] += nv_dpp<0xB1>(v[i]);
    v[i] += nv_dpp<0x4E>(v[i]);
    v[i] += nv_dpp<0x141>(v[i]);
    v[i] += nv_dpp<0x140>(v[i]);
  }
  return v;
}

// The four bias vectors of a net summed over the 16 samples of each component group at once: a reduce-scatter
// butterfly over the 16 values (b0..b3, registers 0..3) — row mirror, half-row mirror, quad xor 2, quad xor 1,
// each stage keeping the half of the values selected by one lane bit — leaves lane s with the total of value s
// (45 VALU instead of 4 x nv_sum16). Written to r[16 (s / 4) + 4 g + s % 4] (b_{s/4} by position).
__device__ __forceinline__ void nv_put_bias4(float* r, const NvLane& ln, const f32x4& b0, const f32x4& b1,
                                             const f32x4& b2, const f32x4& b3) {
  float v[16];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    v[c] = b0[c];
    v[4 + c] = b1[c];
    v[8 + c] = b2[c];
    v[12 + c] = b3[c];
  }
  auto stage = [&](auto dpp, int half, bool hi) {
#pragma unroll
    for (int i = 0; i < half; ++i) {
      const float send = hi ? v[i] : v[i + half], keep = hi ? v[i + half] : v[i];
      v[i] = keep + dpp(send);
    }
  };
  stage([](float x) { return nv_dpp<0x140>(x); }, 8, (ln.s & 8) != 0);  // partner 15 - s (row mirror)
  stage([](float x) { return nv_dpp<0x141>(x); }, 4, (ln.s & 4) != 0);  // partner s ^ 7 (half-row mirror)
  stage([](float x) { return nv_dpp<0x4E>(x); }, 2, (ln.s & 2) != 0);   // s ^ 2
  stage([](float x) { return nv_dpp<0xB1>(x); }, 1, (ln.s & 1) != 0);   // s ^ 1
  r[(ln.s >> 2) * 16 + 4 * ln.g + (ln.s & 3)] = v[0];
}

// A wave's partials into its LDS flush block: matrices in the accumulator layout (row 4g + i,
// column s), vectors summed over samples.
__device__ __forceinline__ void nv_put_mat(float* r, const NvLane& ln, const f32x4& m) {
#pragma unroll
  for (int i = 0; i < 4; ++i) r[(4 * ln.g + i) * 16 + ln.s] = m[i];
}
// Compact matrix put (NvC): row 4g + i -> row map R (-1: padding), column s -> column map C, width NC.
template <int NC, typename RM, typename CM>
__device__ __forceinline__ void nv_put_cmat(float* r, const NvLane& ln, const f32x4& m, RM rm, CM cm) {
  const int c = cm(ln.s);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int q = rm(4 * ln.g + i);
    if (q >= 0 && c >= 0) r[q * NC + c] = m[i];
  }
}
__device__ __forceinline__ void nv_put_vec(float* r, const NvLane& ln, const f32x4& v) {
  const f32x4 t = nv_sum16(v);
  if (ln.s == 0) *reinterpret_cast<f32x4*>(r + 4 * ln.g) = t;
}
template <bool PK>
__device__ __forceinline__ void nv_put_net(float* r, const NvLane& ln, const NvNetAcc& a) {
  using C = NvC<PK>;
  auto all = [](int p) { return p; };
  auto hid = [](int p) { return PK ? ((p & 3) < 2 ? 2 * (p >> 2) + (p & 1) : -1) : (p < 8 ? p : -1); };  // h0 unit
  if constexpr (PK) {
    nv_put_cmat<8>(r + C::W0T, ln, a.w0t, all, hid);
  } else {
    nv_put_cmat<8>(r + C::W0T, ln, a.w0t, all, hid);
    nv_put_cmat<8>(r + C::W0X, ln, a.w0x, [](int p) { return p < 8 ? p : -1; }, hid);
  }
  nv_put_cmat<16>(r + C::W1, ln, a.w1, hid, all);
  nv_put_cmat<16>(r + C::W2, ln, a.w2, all, all);
  if constexpr (PK)
    nv_put_cmat<4>(r + C::W3, ln, a.w3, all, [](int p) { return (p & 3) == 0 ? p >> 2 : -1; });
  else
    nv_put_cmat<8>(r + C::W3, ln, a.w3, all, [](int p) { return p < 8 ? p : -1; });
  static_assert(C::B1 == C::B0 + 16 && C::B2 == C::B1 + 16 && C::B3 == C::B2 + 16, "bias vectors contiguous");
  nv_put_bias4(r + C::B0, ln, a.b0, a.b1, a.b2, a.b3);
}

// Flat (reference-order) parameter f of one BasicMLP -> its index in the compact net block (NvC).
template <bool PK>
__host__ __device__ __forceinline__ int nv_cb_src(int f, int d, int n_t) {
  using C = NvC<PK>;
  const int n_in = d + n_t;
  if (f < n_in * 8) {
    const int r = f / 8, o = f - r * 8;
    if (PK) return C::W0T + (r < d ? 4 * r : 4 * ((r - d) / 3) + 1 + (r - d) % 3) * 8 + o;
    return r < d ? C::W0X + r * 8 + o : C::W0T + (r - d) * 8 + o;
  }
  f -= n_in * 8;
  if (f < 8) return C::B0 + (PK ? 4 * (f / 2) + f % 2 : f);
  f -= 8;
  if (f < 128) return C::W1 + f;  // [h0 unit][16]
  f -= 128;
  if (f < 16) return C::B1 + f;
  f -= 16;
  if (f < 256) return C::W2 + f;
  f -= 256;
  if (f < 16) return C::B2 + f;
  f -= 16;
  if (f < 16 * d) return C::W3 + (f / d) * (PK ? 4 : 8) + f % d;
  f -= 16 * d;
  return C::B3 + (PK ? 4 * f : f);
}

// Slab-row layout of the gradient kernel: [L compact layer blocks (NvC::LAYER each) | time embedding (reference
// order) | loss], row stride rounded up to 4 floats (the layer blocks are stored as float4).
struct NvSlabMap {
  int d, n_t, pk, n_layers;
  int64_t layer_stride, temb_params, n_params, cb;
};
__host__ __device__ __forceinline__ int64_t nv_slab_col(const NvSlabMap& m, int64_t c) {
  const int64_t lcb = (int64_t)m.n_layers * m.cb;
  if (c >= m.n_params) return lcb + m.temb_params;  // loss
  if (c < m.temb_params) return lcb + c;
  c -= m.temb_params;
  const int64_t l = c / m.layer_stride;
  int k = (int)(c - l * m.layer_stride);
  const int64_t base = l * m.cb;
  if (k < m.d) return base + (m.pk ? NvC<true>::SF + 4 * k : NvC<false>::SF + k);  // sf by position
  k -= m.d;
  const int mlp_n = (m.d + m.n_t) * 8 + 8 + 8 * 16 + 16 + 16 * 16 + 16 + 16 * m.d + m.d;
  const int net = k >= mlp_n ? 1 : 0;
  k -= net * mlp_n;
  if (m.pk) return base + (net ? NvC<true>::TNET : NvC<true>::SNET) + nv_cb_src<true>(k, m.d, m.n_t);
  return base + (net ? NvC<false>::TNET : NvC<false>::SNET) + nv_cb_src<false>(k, m.d, m.n_t);
}
__host__ __device__ __forceinline__ int64_t nv_slab_ld(const NvSlabMap& m) {
  return ((int64_t)m.n_layers * m.cb + m.temb_params + 1 + 3) / 4 * 4;
}

// Raw coupling-layer parameter k (reference order: sf, s-net, t-net) -> its LDS position(s) in the padded layer
// image: dst | dstT << 16 (the transposed copy of a matrix entry; 0xFFFF for vectors). Layer-invariant, so a
// block computes it once and every staging is a scatter of the prefetched registers through this table.
template <bool PK>
__device__ __forceinline__ uint32_t nv_layer_dst(int k, int d, int n_t) {
  const int n_in = d + n_t, mlp_n = n_in * 8 + 8 + 8 * 16 + 16 + 16 * 16 + 16 + 16 * d + d;
  if (k < d) return (uint32_t)(NvM<PK>::SF + nv_xpos<PK>(k)) | 0xFFFF0000u;
  k -= d;
  const int net = k >= mlp_n ? 1 : 0;
  int f = k - net * mlp_n;
  const int base = net ? NvM<PK>::TNET : NvM<PK>::SNET;
  auto mat = [&](int M, int pr, int pc) {
    return (uint32_t)(base + M + pr * kNvWS + pc) | ((uint32_t)(base + NvM<PK>::TR + M + pc * kNvWS + pr) << 16);
  };
  auto vec = [&](int B, int p) { return (uint32_t)(base + B + p) | 0xFFFF0000u; };
  if (f < n_in * 8) {
    const int r = f / 8, o = f - r * 8;
    if (PK) return mat(NvM<PK>::W0T, r < d ? nv_xpos<PK>(r) : nv_tpos<PK>(r - d), nv_hpos<PK>(o));
    return r < d ? mat(NvM<PK>::W0X, r, o) : mat(NvM<PK>::W0T, r - d, o);
  }
  f -= n_in * 8;
  if (f < 8) return vec(NvM<PK>::B0, nv_hpos<PK>(f));
  f -= 8;
  if (f < 128) return mat(NvM<PK>::W1, nv_hpos<PK>(f / 16), f % 16);
  f -= 128;
  if (f < 16) return vec(NvM<PK>::B1, f);
  f -= 16;
  if (f < 256) return mat(NvM<PK>::W2, f / 16, f % 16);
  f -= 256;
  if (f < 16) return vec(NvM<PK>::B2, f);
  f -= 16;
  if (f < 16 * d) return mat(NvM<PK>::W3, f / d, nv_xpos<PK>(f % d));
  f -= 16 * d;
  return vec(NvM<PK>::B3, nv_xpos<PK>(f));
}

// ---- block-level staging of the two tile kernels (every thread of the block calls; barriers are the caller's) ----
// with_stage: the lane's offsets into the per-wave sample stage (the gradient kernel's weight-gradient products)
__device__ __forceinline__ NvLane nv_lane(int tid, bool with_stage) {
  int lane = tid & 63;
  asm volatile("" : "+v"(lane));  // opaque: keeps per-use address math out of long-lived registers
  NvLane ln;
  ln.g = lane >> 4;
  ln.s = lane & 15;
  ln.sw = with_stage ? ln.s * kNvSS + 4 * (ln.g ^ nv_swz(ln.s)) : 0;
  ln.sr = with_stage ? ln.g * kNvSS + (ln.s ^ (4 * nv_swz(ln.g))) : 0;
  return ln;
}
// padded [16][kNvWS] (and its transpose unless dst_t is null): position (r, c) <- src[rm(r)][cm(c)], 0 where a
// map gives -1
template <typename RM, typename CM>
__device__ __forceinline__ void nv_stage_mat(float* dst, float* dst_t, const float* src, int ld_src, RM rm, CM cm) {
  for (int q = threadIdx.x; q < 16 * kNvWS; q += kBlock) {
    const int r = q / kNvWS, c = q - r * kNvWS;
    const int sr = c < 16 ? rm(r) : -1, sc = c < 16 ? cm(c) : -1;
    dst[q] = (sr >= 0 && sc >= 0) ? src[sr * ld_src + sc] : 0.f;
    if (dst_t) {
      const int tr = c < 16 ? rm(c) : -1, tc = c < 16 ? cm(r) : -1;
      dst_t[q] = (tr >= 0 && tc >= 0) ? src[tr * ld_src + tc] : 0.f;
    }
  }
}
template <typename PM>
__device__ __forceinline__ void nv_stage_vec(float* dst, const float* src, PM m) {
  for (int q = threadIdx.x; q < 16; q += kBlock) {
    const int k = m(q);
    dst[q] = k >= 0 ? src[k] : 0.f;
  }
}
// the time embedding's matrices into the start of the layer image sW, temb at its positions
template <bool PK>
__device__ __forceinline__ void nv_stage_temb(float* sW, const float* params, int E, bool with_transpose) {
  using M = NvM<PK>;
  auto idn = [E](int p) { return p < E ? p : -1; };
  auto tmap = [E](int p) { return nv_tinv<PK>(p, E); };
  nv_stage_mat(sW + M::E_W1, nullptr, params, E, idn, idn);
  nv_stage_vec(sW + M::E_B1, params + E * E, idn);
  nv_stage_mat(sW + M::E_W2, with_transpose ? sW + M::E_W2T : nullptr, params + E * E + E, E, idn, tmap);
  nv_stage_vec(sW + M::E_B2, params + 2 * E * E + E, tmap);
}
// sinusoid table sF[48]: frequency freq(q), sin weight, cos weight of position q (all 0 for q >= E)
template <typename FQ>
__device__ __forceinline__ void nv_stage_sinusoid(float* sF, int E, FQ freq) {
  const int tid = threadIdx.x;
  if (tid < 16) {
    const bool on = tid < E, is_sin = tid < E / 2;
    sF[tid] = on ? freq(tid) : 0.f;
    sF[16 + tid] = on && is_sin ? 1.f : 0.f;
    sF[32 + tid] = on && !is_sin ? 1.f : 0.f;
  }
}
// the nv_layer_dst table, and the layer image zeroed (its padding is never written again)
template <bool PK>
__device__ __forceinline__ void nv_stage_init(uint32_t* sDst, float* sW, int64_t layer_stride, int d, int n_t) {
  for (int k = threadIdx.x; k < layer_stride; k += kBlock) sDst[k] = nv_layer_dst<PK>(k, d, n_t);
  for (int q = threadIdx.x; q < NvM<PK>::LAYER; q += kBlock) sW[q] = 0.f;
}
// layer l's mask by position, padded with 1
template <bool PK>
__device__ __forceinline__ void nv_stage_mask(float* sW, const NvpArgs& a, int l, int d) {
  const int tid = threadIdx.x;
  if (tid < 16) {
    const int k = nv_xinv<PK>(tid, d);
    sW[NvM<PK>::MASK + tid] = k >= 0 ? a.masks[l * d + k] : 1.f;
  }
}

// ---- blocks of the tile kernels' bodies (gradient, map, score), each defined once. State goes in by reference or
// parameter, never by capture (a captured x cost the identity-layout gradient kernel 12 bytes of scratch); every one
// is inlined. DESIGN.md §13.2 lists the blocks that stay written out in a kernel, and why. ----
// Coupling layer l's raw parameters into registers: one coalesced load per thread and slot, in flight under the
// previous layer's math.
__device__ __forceinline__ void nv_prefetch(float (&pre)[kNvPre], const float* layers, int l, int64_t layer_stride) {
  const float* lp = layers + (int64_t)l * layer_stride;
  const int tid = threadIdx.x;
#pragma unroll
  for (int k = 0; k < kNvPre; ++k) {
    const int q = tid + k * kBlock;
    pre[k] = q < layer_stride ? lp[q] : 0.f;
  }
}
// The prefetched parameters into the layer image sW through the sDst table (nv_layer_dst). WITH_T: with the
// transposed copies that the input-gradient products read; without, the forward entries only. Every thread of the
// block calls; the barriers around it are the caller's.
template <bool WITH_T>
__device__ __forceinline__ void nv_scatter_layer(float* sW, const uint32_t* sDst, const float (&pre)[kNvPre],
                                                 int64_t layer_stride) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int k = 0; k < kNvPre; ++k) {
    const int q = tid + k * kBlock;
    if (q < layer_stride) {
      const uint32_t t = sDst[q];
      sW[t & 0xFFFFu] = pre[k];
      if (WITH_T && (t >> 16) != 0xFFFFu) sW[t >> 16] = pre[k];
    }
  }
}
// The masked input x m of a layer's nets. Packed layout: the coordinates live in register 0 only.
template <bool PK>
__device__ __forceinline__ void nv_masked(const NvV& x, const f32x4& m, NvV& xm) {
#pragma unroll
  for (int u = 0; u < kNvT; ++u) xm[u] = PK ? f32x4{x[u][0] * m[0], 0.f, 0.f, 0.f} : x[u] * m;
}
// Sum of a per-sample value over the four lane groups (lanes s, 16 + s, 32 + s, 48 + s), in every one of them
__device__ __forceinline__ float nv_group_sum(float v) {
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}

template <bool PK>
__global__ __launch_bounds__(kBlock, PK ? kNvWavesPk : kNvWaves) void realnvp_grad_kernel(NvpArgs a, int d, const float* __restrict__ params,
                                                                 const float* __restrict__ tv, int64_t t_stride,
                                                                 const float* __restrict__ xv, int64_t n, int64_t ld,
                                                                 int64_t layer_stride, int64_t n_params,
                                                                 int64_t tile0, float* __restrict__ slab,
                                                                 int64_t slab_ld) {
  // current coupling layer (padded); the time embedding's matrices at its start before the first / after the last
  __shared__ float sW[NvM<PK>::LAYER];
  __shared__ float sF[48];              // sinusoid table: frequency, sin weight, cos weight
  __shared__ float sB[16 + 16 * 16];    // base mean, inverse covariance (0-padded)
  // per-wave sample stages and flush blocks (NvScr)
  __shared__ float sScr[kWavesPerBlock][NvScr<PK>::SIZE];
  __shared__ uint32_t sDst[kNvRaw];                  // raw layer parameter -> LDS position(s), nv_layer_dst
  using C = NvC<PK>;
  const int E = a.E;
  const int n_in = a.in_dim, n_t = n_in - d;
  const int64_t lcb = (int64_t)a.n_layers * C::LAYER;  // slab-row offset of the time-embedding columns
  const int64_t temb_params = nvp_temb_params(E);
  const float* layers = params + temb_params;
  const bool hard = !a.ignore_time && a.soft_init == 0.f;
  const int tid = threadIdx.x, wave = tid >> 6;
  const NvLane ln = nv_lane(tid, true);
  float* const scr = sScr[wave];  // the wave's sample stage, then its flush block (NvScr)
  // ---- per-block tables ----
  nv_stage_sinusoid(sF, E, [E](int q) {  // fp32 on the device (the time kernels: NvFreq)
    const int half = E / 2;
    const float step = logf(10000.f) / (float)(half - 1);
    return expf(-step * (float)(q < half ? q : q - half));
  });
  nv_stage_init<PK>(sDst, sW, layer_stride, d, n_t);
  for (int q = tid; q < 16 + 256; q += kBlock) {  // mean at the x positions; inv_cov rows by position, columns by coordinate
    float v = 0.f;
    if (q < 16) {
      const int k = nv_xinv<PK>(q, d);
      v = k >= 0 ? a.mean[k] : 0.f;
    } else {
      const int r = nv_xinv<PK>((q - 16) / 16, d), c = (q - 16) % 16;
      v = (r >= 0 && c < d) ? a.inv_cov[r * d + c] : 0.f;
    }
    sB[q] = v;
  }
  // Layer parameters are prefetched one staged layer ahead into registers (one coalesced load per
  // thread and slot, in flight under the previous layer's math) and scattered into the padded /
  // transposed layer image through the sDst table. Staging order: L-1 .. 0 (likelihood), 0 .. L-1.
  float pre[kNvPre];
  int staged = 0;  // layers staged so far
  auto stage_layer = [&](int l) {
    __syncthreads();  // every wave is done with the previous layer
    nv_stage_mask<PK>(sW, a, l, d);
    nv_scatter_layer<true>(sW, sDst, pre, layer_stride);
    ++staged;
    if (staged < 2 * a.n_layers)
      nv_prefetch(pre, layers, staged < a.n_layers ? a.n_layers - 1 - staged : staged - a.n_layers, layer_stride);
    __syncthreads();
  };
  nv_prefetch(pre, layers, a.n_layers - 1, layer_stride);
  float* row = slab + (int64_t)blockIdx.x * slab_ld;
  // write this block's reduced partials for the flat range [off, off + len): src(f) -> flush index
  auto flush = [&](int64_t off, int len, auto src) {
    __syncthreads();  // every wave's partials are in its flush block
    for (int f = tid; f < len; f += kBlock) {
      const int k = src(f);
      float v = 0.f;
      if (k >= 0) v = ((sScr[0][k] + sScr[1][k]) + sScr[2][k]) + sScr[3][k];
      row[off + f] = v;
    }
    __syncthreads();  // the flush blocks are free again
  };

  // ---- the wave's tiles ----
  NvV x, gx, temb, gtemb;
  float tt[kNvT], w[kNvT], ldj[kNvT];
  const int64_t base = (tile0 + blockIdx.x) * kNvSPB + wave * 16 * kNvT;
  __syncthreads();  // sW zeroed
  if (E > 0) nv_stage_temb<PK>(sW, params, E, true);
  __syncthreads();
#pragma unroll
  for (int u = 0; u < kNvT; ++u) {
    const int64_t i = base + 16 * u + ln.s;
    const bool active = i < n;
    w[u] = active ? 1.f : 0.f;
    tt[u] = active ? tv[i * t_stride] : 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int k = nv_xinv<PK>(4 * ln.g + c, d);
      x[u][c] = (active && k >= 0 && (!PK || c == 0)) ? xv[i * ld + k] : 0.f;  // packed: registers 1..3 are 0
      gtemb[u][c] = 0.f;
    }
    ldj[u] = 0.f;
  }
  // TimeEmbedding (:8-22): se = SinusoidalEmbedding(t) (:24-38), he = act(se W1 + b1), temb = he W2 + b2
  auto sinusoid = [&](NvV& se) {
#pragma unroll
    for (int u = 0; u < kNvT; ++u)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int q = 4 * ln.g + c;
        const float e = tt[u] * sF[q];
        se[u][c] = sF[16 + q] * sinf(e) + sF[32 + q] * cosf(e);
      }
  };
  // Packed layout: the coordinates live in register 0 only (registers 1..3 of x, gx stay exactly 0 through
  // every coupling layer), so the per-coordinate coupling math runs over NC = 1 register.
  constexpr int NC = PK ? 1 : 4;
  // sf = e^alpha and 1 / sf of the staged layer
  auto scale = [&](f32x4& sf, f32x4& isf) {
    const f32x4 sfw = nv_vec(sW + NvM<PK>::SF, ln);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      sf[c] = nv_exp(sfw[c]);
      isf[c] = __builtin_amdgcn_rcpf(sf[c]);
    }
  };
  if (E > 0) {
    NvV se, he;
    sinusoid(se);
    nv_bcast(he, nv_vec(sW + NvM<PK>::E_B1, ln));
    nv_fwdT(sW + NvM<PK>::E_W1, ln, se, he);
#pragma unroll
    for (int u = 0; u < kNvT; ++u) he[u] = nv_celu4(he[u]);
    nv_bcast(temb, nv_vec(sW + NvM<PK>::E_B2, ln));
    nv_fwdT(sW + NvM<PK>::E_W2, ln, he, temb);
    __syncthreads();  // every wave has read the time embedding: back to the zero-padded layer image
    for (int q = tid; q < NvM<PK>::TEMB; q += kBlock) sW[q] = 0.f;
  } else {
#pragma unroll
    for (int u = 0; u < kNvT; ++u)
#pragma unroll
      for (int c = 0; c < 4; ++c) temb[u][c] = (!a.ignore_time && 4 * ln.g + c == nv_tpos<PK>(0)) ? tt[u] : 0.f;
  }
  // ---- likelihood pass (layers L-1 .. 0): x <- (x + tr) e^s ----
  for (int l = a.n_layers - 1; l >= 0; --l) {
    stage_layer(l);
    const f32x4 m = nv_vec(sW + NvM<PK>::MASK, ln);
    f32x4 sf, isf;
    scale(sf, isf);
    NvV xm, so, to;
    nv_masked<PK>(x, m, xm);
    {
      NvAct h;
      nv_mlp_fwd<PK>(sW + NvM<PK>::SNET, ln, temb, xm, h, so);
      nv_mlp_fwd<PK>(sW + NvM<PK>::TNET, ln, temb, xm, h, to);
    }
#pragma unroll
    for (int u = 0; u < kNvT; ++u) {
#pragma unroll
      for (int c = 0; c < NC; ++c) {  // padded / masked k: keep = 0, x unchanged
        const float keep = 1.f - m[c];
        const float sk = nv_tanh((hard ? tt[u] * so[u][c] : so[u][c]) * isf[c]) * sf[c] * keep;
        x[u][c] = (x[u][c] + (hard ? tt[u] * to[u][c] : to[u][c]) * keep) * nv_exp(sk);
        ldj[u] += sk;
      }
    }
  }
  // ---- base density log p0(x0) and its gradient (per-wave stage holds the tile's x rows) ----
  float lsum = 0.f;  // sum over the wave's samples of w log p (lane-partial)
#pragma unroll
  for (int u = 0; u < kNvT; ++u) {
    const f32x4 diff = x[u] - nv_vec(sB, ln);
    nv_wave_sync();
    *reinterpret_cast<f32x4*>(scr + ln.sw) = diff;
    nv_wave_sync();
    float quad = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int r = 4 * ln.g + c;
      float acc = 0.f;
      for (int q = 0; q < d; ++q)
        acc = fmaf(sB[16 + r * 16 + q], scr[ln.s * kNvSS + (nv_xpos<PK>(q) ^ (4 * nv_swz(ln.s)))], acc);
      quad = fmaf(diff[c], acc, quad);
      gx[u][c] = PK && c > 0 ? 0.f : -w[u] * acc;
    }
    const float part = nv_group_sum(ldj[u] - 0.5f * quad);  // the four groups' parts sum to log p + 0.5 log_det
    if (ln.g == 0) lsum += w[u] * (part - 0.5f * a.log_det);
  }
  // ---- backward through layers 0 .. L-1, rebuilding each layer's input ----
  for (int l = 0; l < a.n_layers; ++l) {
    stage_layer(l);
    const f32x4 m = nv_vec(sW + NvM<PK>::MASK, ln);
    f32x4 sfv, isf;
    scale(sfv, isf);
    NvNetAcc as, at;
    as.zero();
    at.zero();
    f32x4 galpha = {0.f, 0.f, 0.f, 0.f};
    NvV xm, out, s, es, gso, gto, gacc;
    NvAct h;
    nv_masked<PK>(x, m, xm);
    nv_mlp_fwd<PK>(sW + NvM<PK>::SNET, ln, temb, xm, h, out);
#pragma unroll
    for (int u = 0; u < kNvT; ++u) {
      gso[u] = gto[u] = gacc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const float keep = 1.f - m[c];
        const float spre = hard ? tt[u] * out[u][c] : out[u][c];
        const float sf = sfv[c];
        const float th = nv_tanh(spre * isf[c]);
        s[u][c] = th * sf * keep;
        es[u][c] = nv_exp(s[u][c]);
        const float gs = (gx[u][c] * x[u][c] + w[u]) * keep;  // d(log p0 + ldj)/ds via x_out and ldj
        const float dth = 1.f - th * th;
        galpha[c] += gs * (th * sf - dth * spre);              // d/d scaling_factor (sf = e^alpha)
        gso[u][c] = (hard ? tt[u] : 1.f) * gs * dth;           // d/d scale_net output
        gto[u][c] = (hard ? tt[u] : 1.f) * gx[u][c] * es[u][c] * keep;  // d/d translate_net output
      }
    }
    nv_mlp_bwd<PK>(sW + NvM<PK>::SNET, ln, scr, temb, xm, h, gso, as, gtemb, gacc);
    nv_put_vec(scr + NvScr<PK>::TR + NvC<PK>::NET, ln, galpha);  // behind the stage (nv_flush_lds)
    nv_put_net<PK>(scr + NvScr<PK>::TR, ln, as);
    nv_mlp_fwd<PK>(sW + NvM<PK>::TNET, ln, temb, xm, h, out);
    nv_mlp_bwd<PK>(sW + NvM<PK>::TNET, ln, scr, temb, xm, h, gto, at, gtemb, gacc);
#pragma unroll
    for (int u = 0; u < kNvT; ++u)
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const float tr = (hard ? tt[u] * out[u][c] : out[u][c]) * (1.f - m[c]);
        x[u][c] = x[u][c] * __builtin_amdgcn_rcpf(es[u][c]) - tr;
        gx[u][c] = gx[u][c] * es[u][c] + m[c] * gacc[u][c];
      }
    // the t-net partials into the wave's compact block (it aliases only the wave's own stage: no barrier), then
    // the block's four wave blocks summed as float4 into the layer's slab-row segment. The next stage_layer's
    // barrier orders these reads before any wave's next stage writes.
    nv_wave_sync();
    nv_put_net<PK>(scr + C::TNET, ln, at);
    __syncthreads();
    for (int q = tid; q < C::LAYER / 4; q += kBlock) {
      const int o = nv_flush_lds<PK>(4 * q);
      const f32x4 v = ((*reinterpret_cast<const f32x4*>(&sScr[0][o]) + *reinterpret_cast<const f32x4*>(&sScr[1][o])) +
                       *reinterpret_cast<const f32x4*>(&sScr[2][o])) +
                      *reinterpret_cast<const f32x4*>(&sScr[3][o]);
      *reinterpret_cast<f32x4*>(row + (int64_t)l * C::LAYER + 4 * q) = v;
    }
  }
  __syncthreads();  // the last layer's sums are read: the stages and the layer image are free again
  if (E > 0) {
    nv_stage_temb<PK>(sW, params, E, true);
    __syncthreads();
  }
  // ---- time-embedding backward and the loss column ----
  if (E > 0) {
    f32x4 w1 = {0.f, 0.f, 0.f, 0.f}, w2 = w1, b1 = w1, b2 = w1;
    NvV se, he, gz;
    // se and he again (the forward kept neither). Sinusoid and hidden layer stay two steps written out at both
    // places: as one local, lambda or function, they cost the packed kernel 3 more spilled dwords (168 VGPRs).
    sinusoid(se);
    nv_bcast(he, nv_vec(sW + NvM<PK>::E_B1, ln));
    nv_fwdT(sW + NvM<PK>::E_W1, ln, se, he);
#pragma unroll
    for (int u = 0; u < kNvT; ++u) he[u] = nv_celu4(he[u]);
    w2 = nv_wgrad(scr, ln, he, gtemb, w2);
    nv_bcast(gz, f32x4{0.f, 0.f, 0.f, 0.f});
    nv_fwdT(sW + NvM<PK>::E_W2T, ln, gtemb, gz);
#pragma unroll
    for (int u = 0; u < kNvT; ++u) {
      b2 += gtemb[u];
      gz[u] = nv_dact4(gz[u], he[u]);
      b1 += gz[u];
    }
    w1 = nv_wgrad(scr, ln, se, gz, w1);
    __syncthreads();  // stages done (flush blocks alias them)
    nv_put_mat(scr + 0, ln, w1);
    nv_put_vec(scr + 256, ln, b1);
    nv_put_mat(scr + 272, ln, w2);
    nv_put_vec(scr + 528, ln, b2);
    const int EE = E * E + E;
    flush(lcb, 2 * EE, [&](int f) {
      const int part = f >= EE, r = f - part * EE;
      const int o = part * 272;  // W2 / b2 columns at the temb positions
      if (r < E * E) return o + (r / E) * 16 + (part ? nv_tpos<PK>(r % E) : r % E);
      return o + 256 + (part ? nv_tpos<PK>(r - E * E) : r - E * E);
    });
  }
  lsum += __shfl_xor(lsum, 1, 64);
  lsum += __shfl_xor(lsum, 2, 64);
  lsum += __shfl_xor(lsum, 4, 64);
  lsum += __shfl_xor(lsum, 8, 64);
  if (tid % 64 == 0) scr[0] = lsum;
  flush(lcb + temb_params, 1, [&](int) { return 0; });
}

// Slab column sums in two fixed-order fp64 stages (bit-reproducible): kNvSplits row splits of the
// chunk, each summed by 4 row phases of a 64-column block (4 independent loads in flight per
// lane), then the splits in order. Column c of parts is reference parameter c (n_params: the loss),
// read from slab column nv_slab_col(c). On the last chunk grad[c] = scale * acc[c] (c < n_params) and
// loss = scale * acc[n_params].
constexpr int kNvSplits = 16;
__global__ __launch_bounds__(kBlock) void nvp_slab_split_kernel(const float* __restrict__ slab_base, int rows,
                                                                 int64_t ld, NvSlabMap map, int64_t n_cols,
                                                                 double* __restrict__ parts) {
  __shared__ double part[kBlock];
  const int64_t c = (int64_t)blockIdx.x * 64 + (threadIdx.x & 63);
  const float* slab = slab_base + (c < n_cols ? nv_slab_col(map, c) : 0);
  const int g = threadIdx.x >> 6;
  const int rps = (rows + kNvSplits - 1) / kNvSplits;
  const int r0 = blockIdx.y * rps, r1 = r0 + rps < rows ? r0 + rps : rows;
  double acc = 0.0;
  if (c < n_cols) {
    int r = r0 + g;
    for (; r + 12 < r1; r += 16) {
      const float v0 = slab[(int64_t)r * ld], v1 = slab[(int64_t)(r + 4) * ld];
      const float v2 = slab[(int64_t)(r + 8) * ld], v3 = slab[(int64_t)(r + 12) * ld];
      acc += (double)v0;
      acc += (double)v1;
      acc += (double)v2;
      acc += (double)v3;
    }
    for (; r < r1; r += 4) acc += (double)slab[(int64_t)r * ld];
  }
  part[threadIdx.x] = acc;
  __syncthreads();
  if (g == 0 && c < n_cols)
    parts[blockIdx.y * n_cols + c] =
        ((part[threadIdx.x] + part[threadIdx.x + 64]) + part[threadIdx.x + 128]) + part[threadIdx.x + 192];
}

__global__ __launch_bounds__(kBlock) void nvp_grad_reduce_kernel(const double* __restrict__ parts,
                                                                  int64_t n_params, double* acc64,
                                                                  int first, int last, double scale,
                                                                  float* __restrict__ grad,
                                                                  float* __restrict__ loss) {
  const int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (c <= n_params) {
    double v = 0.0;
#pragma unroll
    for (int q = 0; q < kNvSplits; ++q) v += parts[q * (n_params + 1) + c];
    if (!first) v += acc64[c];
    acc64[c] = v;
    if (last) {
      if (c < n_params) grad[c] = (float)(scale * v);
      else *loss = (float)(scale * v);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Time derivatives of the log-density: (log p_t(x), d/dt, d2/dt2) per sample in one pass, by second-order
// forward mode in t through the whole model (the KMV residual's weight c = ds2 + ds^2 + gamma ds,
// kinetic_mckean_vlasov.py:57-72, 86-91, for a learned density; the reference takes jax.grad(., 0) twice).
// Every t-dependent quantity is three streams [value, d/dt, d2/dt2]: dense layers act on the three alike
// (bias on the value only: one weight fetch feeds three FMAs), y = g(z) maps them by
//   y' = g'(z) z',  y'' = g''(z) z'^2 + g'(z) z'',
// products by Leibniz. Kinks: relu g' = [z > 0], g'' = 0; celu / elu (g', g'') = (1, 0) for z > 0 and
// (e^z, e^z) for z <= 0. General path: one thread per sample on the VALU, like realnvp_logdensity_kernel
// (weights at wave-uniform addresses); every register array is indexed by unrolled loop counters only (the
// runtime widths E and in_dim guard wave-uniform branches). Plain stores, no atomics: deterministic.
// ---------------------------------------------------------------------------------------------
// (g(z), g'(z), g''(z)) on the hardware exp2 / rcp
// (ACT is a template parameter down to here: a runtime switch is if-converted into all seven evaluations)
template <int ACT>
__device__ __forceinline__ void nvp_act_d2(float z, float& g, float& g1, float& g2) {
  switch (ACT) {
    case PDEINV_ACT_CELU:
    case PDEINV_ACT_ELU: {
      const float e = nv_exp(fminf(z, 0.f));
      const bool pos = z > 0.f;
      g = pos ? z : e - 1.f;
      g1 = pos ? 1.f : e;
      g2 = pos ? 0.f : e;
      break;
    }
    case PDEINV_ACT_RELU:
      g = fmaxf(z, 0.f);
      g1 = z > 0.f ? 1.f : 0.f;
      g2 = 0.f;
      break;
    case PDEINV_ACT_TANH:
      g = nv_tanh(z);
      g1 = 1.f - g * g;
      g2 = -2.f * g * g1;
      break;
    case PDEINV_ACT_SILU: {
      const float s = __builtin_amdgcn_rcpf(1.f + nv_exp(-z)), q = s * (1.f - s);
      g = z * s;
      g1 = fmaf(z, q, s);
      g2 = q * fmaf(z, 1.f - 2.f * s, 2.f);
      break;
    }
    case PDEINV_ACT_SOFTPLUS: {
      const float s = __builtin_amdgcn_rcpf(1.f + nv_exp(-z));
      g = fmaxf(z, 0.f) + log1pf(nv_exp(-fabsf(z)));
      g1 = s;
      g2 = s * (1.f - s);
      break;
    }
    default: {  // gelu, tanh approximation: g = z (1 + tanh u) / 2, u = c (z + a z^3)
      const float c = 0.7978845608028654f, a = 0.044715f;
      const float u = c * (z + a * z * z * z), u1 = c * fmaf(3.f * a * z, z, 1.f), u2 = 6.f * c * a * z;
      const float th = nv_tanh(u), q = 1.f - th * th;
      const float th1 = q * u1, th2 = q * u2 - 2.f * th * q * u1 * u1;
      g = 0.5f * z * (1.f + th);
      g1 = 0.5f * (1.f + th) + 0.5f * z * th1;
      g2 = fmaf(0.5f * z, th2, th1);
    }
  }
}

// y = g(z) on the three streams, in place: y' = g' z', y'' = g'' z'^2 + g' z''
template <int ACT>
__device__ __forceinline__ void nvp_act3(float& z0, float& z1, float& z2) {
  float g, g1, g2;
  nvp_act_d2<ACT>(z0, g, g1, g2);
  z0 = g;
  z2 = fmaf(g2 * z1, z1, g1 * z2);
  z1 = g1 * z1;
}

// The three streams of a dense layer out = act?(b + in @ W) in pieces: bias (value stream only), the rows of one
// input block (rows i >= n_in of the NI-wide block are not read; one weight fetch feeds three FMAs), activation.
template <int NO>
__device__ __forceinline__ void dense3_bias(const float* __restrict__ b, float (&out)[3][NO]) {
#pragma unroll
  for (int o = 0; o < NO; ++o) {
    out[0][o] = b[o];
    out[1][o] = 0.f;
    out[2][o] = 0.f;
  }
}
template <int NI, int NO>
__device__ __forceinline__ void dense3_rows(const float* __restrict__ W, const float (&in)[3][NI], int n_in,
                                            float (&out)[3][NO]) {
  asm volatile("" ::: "memory");  // no weight fetches hoisted across dense layers (register pressure)
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    if (i < n_in) {
#pragma unroll
      for (int o = 0; o < NO; ++o) {
        const float w = W[i * NO + o];
        out[0][o] = fmaf(in[0][i], w, out[0][o]);
        out[1][o] = fmaf(in[1][i], w, out[1][o]);
        out[2][o] = fmaf(in[2][i], w, out[2][o]);
      }
    }
  }
}
template <int ACT, int NO>
__device__ __forceinline__ void dense3_act(float (&out)[3][NO]) {
#pragma unroll
  for (int o = 0; o < NO; ++o) nvp_act3<ACT>(out[0][o], out[1][o], out[2][o]);
}

// BasicMLP over the input [xm (D) | temb (n_t)] kept as its two blocks
template <int D, int ACT>
__device__ __forceinline__ const float* basic_mlp3(const float* p, const float (&xm)[3][D], const float (&temb)[3][16],
                                                   int n_t, float (&out)[3][D]) {
  float h0[3][8], h1[3][16], h2[3][16];
  const int n_in = D + n_t;
  dense3_bias<8>(p + n_in * 8, h0);
  dense3_rows<D, 8>(p, xm, D, h0);
  dense3_rows<16, 8>(p + D * 8, temb, n_t, h0);
  dense3_act<ACT, 8>(h0);
  p += n_in * 8 + 8;
  dense3_bias<16>(p + 8 * 16, h1);
  dense3_rows<8, 16>(p, h0, 8, h1);
  dense3_act<ACT, 16>(h1);
  p += 8 * 16 + 16;
  dense3_bias<16>(p + 16 * 16, h2);
  dense3_rows<16, 16>(p, h1, 16, h2);
  dense3_act<ACT, 16>(h2);
  p += 16 * 16 + 16;
  dense3_bias<D>(p + 16 * D, out);
  dense3_rows<16, D>(p, h2, 16, out);
  return p + 16 * D + D;
}

// Frequencies of the sinusoidal embedding by position (q and q + E / 2: 10000^(-q / (E / 2 - 1))), rounded once from
// fp64 on the host. Computed in fp32 (expf(-step q)) they carry a few 1e-7 of relative error, the same for every
// layer: harmless for the value, but a time-scale error dt_eff that shows in the derivatives as dt2 * dt_eff.
struct NvFreq {
  float w[16];
};

// The two formulas that both time kernels must evaluate alike, each defined once. They are statement macros, not
// functions: called from realnvp_time_kernel as __forceinline__ functions (array, scalar-reference, by-value and
// restrict-free signatures were tried) the same text changes that kernel's instruction stream, with the same
// resource table but more SGPR spills, and costs it 0.5 - 1 % (d = 4, 7, 8); expanded in place both kernels
// compile to the instructions they had. Arguments are evaluated more than once (pass plain variables or array
// elements); the macros' own names end in _ so that they capture none of the caller's.
//
// NVP_COUPLE3: the coupling update of one coordinate of one sample on the three streams: x <- (x + tr keep) e^{sk},
// sk = tanh(s / sf) sf keep, ldj += sk, with s and tr the nets' outputs (times t under the hard parameterisation).
// On the accurate expf / tanhf / division (d per layer, against the nets' hundreds of activations): the three
// streams of x are large and every later layer sees their rounding, so an ulp here is what the derivatives' error
// is made of. S*, T*: the nets' outputs (values); X*, L*: the streams of x and ldj (lvalues).
#define NVP_COUPLE3(t, hard, sf, keep, S0, S1, S2, T0, T1, T2, X0, X1, X2, L0, L1, L2)             \
  do {                                                                                            \
    float s0_ = (S0), s1_ = (S1), s2_ = (S2);                                                     \
    float t0_ = (T0), t1_ = (T1), t2_ = (T2);                                                     \
    if (hard) { /* (t f)' = f + t f', (t f)'' = 2 f' + t f'' */                                   \
      s2_ = fmaf((t), s2_, 2.f * s1_);                                                            \
      s1_ = fmaf((t), s1_, s0_);                                                                  \
      s0_ *= (t);                                                                                 \
      t2_ = fmaf((t), t2_, 2.f * t1_);                                                            \
      t1_ = fmaf((t), t1_, t0_);                                                                  \
      t0_ *= (t);                                                                                 \
    }                                                                                             \
    const float sf_ = (sf);                                                                       \
    const float th_ = tanhf(s0_ / sf_), g1_ = 1.f - th_ * th_;                                    \
    const float k0_ = th_ * sf_ * (keep);                                                         \
    const float k1_ = g1_ * s1_ * (keep);                                                         \
    const float k2_ = g1_ * (s2_ - 2.f * th_ * s1_ * s1_ / sf_) * (keep);                         \
    const float e0_ = expf(k0_), e1_ = e0_ * k1_, e2_ = e0_ * fmaf(k1_, k1_, k2_);                \
    const float y0_ = (X0) + t0_ * (keep), y1_ = (X1) + t1_ * (keep), y2_ = (X2) + t2_ * (keep);  \
    (X0) = y0_ * e0_;                                                                             \
    (X1) = fmaf(y1_, e0_, y0_ * e1_);                                                             \
    (X2) = fmaf(y2_, e0_, fmaf(2.f * y1_, e1_, y0_ * e2_));                                       \
    (L0) += k0_;                                                                                  \
    (L1) += k1_;                                                                                  \
    (L2) += k2_;                                                                                  \
  } while (0)

// NVP_BASE_STORE3: base density and the outputs of sample i: quad = diff^T A diff and its derivatives (A need not be
// symmetric) over the first d of the DMAX coordinates in x[3][DMAX], then (log p, d/dt, d2/dt2) =
// (-0.5 (log_det + q0) + ldj0, -0.5 q1 + ldj1, -0.5 q2 + ldj2); ignore_time writes exact zeros for the derivatives.
// The general path passes DMAX = d = D, the matrix-core path DMAX = 4 and its runtime d.
#define NVP_BASE_STORE3(a, x, DMAX, d, ldj, i, logp, ds)                                         \
  do {                                                                                           \
    float q0_ = 0.f, q1_ = 0.f, q2_ = 0.f;                                                       \
    _Pragma("unroll") for (int r_ = 0; r_ < (DMAX); ++r_) {                                      \
      if (r_ < (d)) {                                                                            \
        float a0_ = 0.f, a1_ = 0.f, a2_ = 0.f;                                                   \
        _Pragma("unroll") for (int c_ = 0; c_ < (DMAX); ++c_) {                                  \
          if (c_ < (d)) {                                                                        \
            const float w_ = (a).inv_cov[r_ * (d) + c_];                                         \
            a0_ = fmaf(w_, (x)[0][c_] - (a).mean[c_], a0_);                                      \
            a1_ = fmaf(w_, (x)[1][c_], a1_);                                                     \
            a2_ = fmaf(w_, (x)[2][c_], a2_);                                                     \
          }                                                                                      \
        }                                                                                        \
        const float d0_ = (x)[0][r_] - (a).mean[r_];                                             \
        q0_ = fmaf(d0_, a0_, q0_);                                                               \
        q1_ = fmaf((x)[1][r_], a0_, fmaf(d0_, a1_, q1_));                                        \
        q2_ = fmaf((x)[2][r_], a0_, fmaf(2.f * (x)[1][r_], a1_, fmaf(d0_, a2_, q2_)));           \
      }                                                                                          \
    }                                                                                            \
    if (logp) (logp)[i] = -0.5f * ((a).log_det + q0_) + (ldj)[0];                                \
    f32x2 o_ = {fmaf(-0.5f, q1_, (ldj)[1]), fmaf(-0.5f, q2_, (ldj)[2])};                         \
    if ((a).ignore_time) o_ = f32x2{0.f, 0.f};                                                   \
    *reinterpret_cast<f32x2*>((ds) + 2 * (i)) = o_;                                              \
  } while (0)

// Sample i: n_rows == 0: (tv[i * t_stride], xv + i * ld); n_rows > 0 (the sets view of pdeinv_kmv_weights):
// set = i / n_rows, row r = i % n_rows: (tv[set], xv + set * set_stride + r * ld). Outputs at index i.
template <int D, int ACT>
__global__ __launch_bounds__(kBlock, 2) void realnvp_time_kernel(NvpArgs a, NvFreq fr, const float* __restrict__ params,
                                                              const float* __restrict__ tv, int64_t t_stride,
                                                              const float* __restrict__ xv, int64_t n, int64_t ld,
                                                              int64_t n_rows, int64_t set_stride,
                                                              int64_t layer_stride, float* __restrict__ logp,
                                                              float* __restrict__ ds) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const int64_t set = n_rows > 0 ? i / n_rows : 0;
  const float t = n_rows > 0 ? tv[set] : tv[i * t_stride];
  const float* xr = n_rows > 0 ? xv + set * set_stride + (i - set * n_rows) * ld : xv + i * ld;
  float x[3][D];
#pragma unroll
  for (int k = 0; k < D; ++k) {
    x[0][k] = xr[k];
    x[1][k] = 0.f;
    x[2][k] = 0.f;
  }
  float temb[3][16];
#pragma unroll
  for (int q = 0; q < 16; ++q) temb[0][q] = temb[1][q] = temb[2][q] = 0.f;
  const float* p = params;
  const int E = a.E;
  if (!a.ignore_time) {
    if (E > 0) {
      const int half = E / 2;
      float se[3][16], h[3][16];
#pragma unroll
      for (int q = 0; q < 16; ++q) {  // position q: sin of frequency q (q < half), cos of frequency q - half
        se[0][q] = se[1][q] = se[2][q] = 0.f;
        if (q < E) {
          const bool is_sin = q < half;
          const float w = fr.w[q];
          float sn, cs;
          sincosf(t * w, &sn, &cs);
          se[0][q] = is_sin ? sn : cs;
          se[1][q] = is_sin ? w * cs : -w * sn;
          se[2][q] = -w * w * se[0][q];
        }
      }
      // two E x E dense layers; unrolled to 16 x 16 with the rows and columns >= E skipped. (A local, not dense3_bias /
      // dense3_rows given a runtime stride and width: that form changes the register allocation of this kernel, whose
      // instruction stream is kept as it was.)
      auto layer = [&](const float* W, const float (&in)[3][16], float (&out)[3][16]) {
#pragma unroll
        for (int o = 0; o < 16; ++o) {
          out[0][o] = o < E ? W[E * E + o] : 0.f;
          out[1][o] = 0.f;
          out[2][o] = 0.f;
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          if (q < E) {
#pragma unroll
            for (int o = 0; o < 16; ++o) {
              if (o < E) {
                const float w = W[q * E + o];
                out[0][o] = fmaf(in[0][q], w, out[0][o]);
                out[1][o] = fmaf(in[1][q], w, out[1][o]);
                out[2][o] = fmaf(in[2][q], w, out[2][o]);
              }
            }
          }
        }
      };
      layer(p, se, h);
#pragma unroll
      for (int o = 0; o < 16; ++o)
        if (o < E) nvp_act3<ACT>(h[0][o], h[1][o], h[2][o]);
      p += E * E + E;
      layer(p, h, temb);
      p += E * E + E;
    } else {
      temb[0][0] = t;
      temb[1][0] = 1.f;
    }
  }
  const float* layers = p;
  const bool hard = !a.ignore_time && a.soft_init == 0.f;
  float ldj[3] = {0.f, 0.f, 0.f};
  for (int l = a.n_layers - 1; l >= 0; --l) {  // likelihood direction: reversed layers
    const float* lp = layers + (int64_t)l * layer_stride;
    const float* m = a.masks + l * D;
    float xm[3][D];
#pragma unroll
    for (int s = 0; s < 3; ++s)
#pragma unroll
      for (int k = 0; k < D; ++k) xm[s][k] = x[s][k] * m[k];
    float sc[3][D], tr[3][D];
    const float* sfp = lp;
    const int n_t = a.in_dim - D;
    const float* q = basic_mlp3<D, ACT>(lp + D, xm, temb, n_t, sc);
    basic_mlp3<D, ACT>(q, xm, temb, n_t, tr);
#pragma unroll
    for (int k = 0; k < D; ++k) {
      const float keep = 1.f - m[k];
      NVP_COUPLE3(t, hard, expf(sfp[k]), keep, sc[0][k], sc[1][k], sc[2][k], tr[0][k], tr[1][k], tr[2][k], x[0][k], x[1][k],
                  x[2][k], ldj[0], ldj[1], ldj[2]);
    }
  }
  NVP_BASE_STORE3(a, x, D, D, ldj, i, logp, ds);
}

// ---------------------------------------------------------------------------------------------
// Matrix-core path of the time derivatives for the reference's flow (celu / elu, packed layout: d <= 4, 4 <= E <= 12,
// time-conditioned). The tile machinery of realnvp_grad_kernel: 16-sample tiles in the v_mfma_f32_16x16x4_f32
// accumulator layout, the LDS weight image NvM<true>, layers chained with no data movement. The three Taylor
// streams are three B operands against one A read (kNvT tiles each: 3 kNvT independent MFMA chains per weight
// fetch); the activation rule is the epilogue between layers; the coupling update, the base form and the outputs
// are the general path's arithmetic (accurate expf / tanhf, NvFreq frequencies), one coordinate per lane group.
// ---------------------------------------------------------------------------------------------
typedef NvV NvV3[3];

template <int JM = 0xF>
__device__ __forceinline__ void nv_fwdT3(const float* W, const NvLane& ln, const NvV3& x, NvV3& c) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (!((JM >> j) & 1)) continue;
    const float av = W[(4 * ln.g + j) * kNvWS + ln.s];
#pragma unroll
    for (int s = 0; s < 3; ++s)
#pragma unroll
      for (int u = 0; u < kNvT; ++u) c[s][u] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, x[s][u][j], c[s][u], 0, 0, 0);
  }
}
__device__ __forceinline__ void nv_bias3(NvV3& z, const f32x4& b) {
#pragma unroll
  for (int u = 0; u < kNvT; ++u) {
    z[0][u] = b;
    z[1][u] = z[2][u] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
}
// celu on the three streams (padding components: z = z' = z'' = 0 -> exactly 0)
__device__ __forceinline__ void nv_celu3(NvV3& z) {
#pragma unroll
  for (int u = 0; u < kNvT; ++u)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float v0 = z[0][u][c], v1 = z[1][u][c], v2 = z[2][u][c];  // (a vector's element binds to no reference)
      nvp_act3<PDEINV_ACT_CELU>(v0, v1, v2);
      z[0][u][c] = v0;
      z[1][u][c] = v1;
      z[2][u][c] = v2;
    }
}
// BasicMLP on the three streams, packed layout: input [xm (register 0) | temb (registers 1..3)]
__device__ __forceinline__ void nv_mlp_fwd3(const float* p, const NvLane& ln, const NvV3& temb, const float (&xm)[3][kNvT],
                                            NvV3& out) {
  using M = NvM<true>;
  NvV3 in, z, h;
#pragma unroll
  for (int s = 0; s < 3; ++s)
#pragma unroll
    for (int u = 0; u < kNvT; ++u) in[s][u] = f32x4{xm[s][u], temb[s][u][1], temb[s][u][2], temb[s][u][3]};
  nv_bias3(z, nv_vec(p + M::B0, ln));
  nv_fwdT3(p + M::W0T, ln, in, z);
  nv_celu3(z);
  nv_bias3(h, nv_vec(p + M::B1, ln));
  nv_fwdT3<0x3>(p + M::W1, ln, z, h);  // h0: 8 units in registers 0, 1
  nv_celu3(h);
  nv_bias3(z, nv_vec(p + M::B2, ln));
  nv_fwdT3(p + M::W2, ln, h, z);
  nv_celu3(z);
  nv_bias3(out, nv_vec(p + M::B3, ln));
  nv_fwdT3(p + M::W3, ln, z, out);
}

constexpr int kNvWavesTime = 2;  // waves per SIMD of the matrix-core time-derivative kernel
__global__ __launch_bounds__(kBlock, kNvWavesTime) void realnvp_time_mfma_kernel(
    NvpArgs a, NvFreq fr, int d, const float* __restrict__ params, const float* __restrict__ tv, int64_t t_stride,
    const float* __restrict__ xv, int64_t n, int64_t ld, int64_t n_rows, int64_t set_stride, int64_t layer_stride,
    float* __restrict__ logp, float* __restrict__ ds) {
  using M = NvM<true>;
  __shared__ float sW[M::LAYER];  // current coupling layer (padded); the time embedding before the first
  __shared__ float sF[48];        // sinusoid table: frequency, sin weight, cos weight
  __shared__ uint32_t sDst[kNvRaw];
  const int E = a.E, n_t = a.in_dim - d;
  const float* layers = params + nvp_temb_params(E);
  const bool hard = a.soft_init == 0.f;
  const int tid = threadIdx.x, wave = tid >> 6;
  const NvLane ln = nv_lane(tid, false);
  nv_stage_sinusoid(sF, E, [&fr](int q) { return fr.w[q]; });  // rounded from fp64 on the host (NvFreq)
  nv_stage_init<true>(sDst, sW, layer_stride, d, n_t);
  __syncthreads();
  nv_stage_temb<true>(sW, params, E, false);
  __syncthreads();
  // ---- the wave's tiles: lane (g, s) holds coordinate g of sample s ----
  float xs[3][kNvT], tt[kNvT], ldj[3][kNvT];
  int64_t idx[kNvT];
  const int64_t base = (int64_t)blockIdx.x * kNvSPB + wave * 16 * kNvT;
#pragma unroll
  for (int u = 0; u < kNvT; ++u) {
    const int64_t i = base + 16 * u + ln.s;
    idx[u] = i < n ? i : -1;
    float t = 0.f, x0 = 0.f;
    if (i < n) {
      const int64_t set = n_rows > 0 ? i / n_rows : 0;
      t = n_rows > 0 ? tv[set] : tv[i * t_stride];
      const float* xr = n_rows > 0 ? xv + set * set_stride + (i - set * n_rows) * ld : xv + i * ld;
      if (ln.g < d) x0 = xr[ln.g];
    }
    tt[u] = t;
    xs[0][u] = x0;
    xs[1][u] = xs[2][u] = 0.f;
    ldj[0][u] = ldj[1][u] = ldj[2][u] = 0.f;
  }
  NvV3 temb;
  {
    NvV3 se, he;
#pragma unroll
    for (int u = 0; u < kNvT; ++u)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int q = 4 * ln.g + c;
        const float w = sF[q], ws = sF[16 + q], wc = sF[32 + q];
        float sn, cs;
        sincosf(tt[u] * w, &sn, &cs);
        const float v0 = ws * sn + wc * cs;
        se[0][u][c] = v0;
        se[1][u][c] = w * (ws * cs - wc * sn);
        se[2][u][c] = -w * w * v0;
      }
    nv_bias3(he, nv_vec(sW + M::E_B1, ln));
    nv_fwdT3(sW + M::E_W1, ln, se, he);
    nv_celu3(he);
    nv_bias3(temb, nv_vec(sW + M::E_B2, ln));
    nv_fwdT3(sW + M::E_W2, ln, he, temb);
  }
  __syncthreads();  // every wave has read the time embedding: back to the zero-padded layer image
  for (int q = tid; q < M::TEMB; q += kBlock) sW[q] = 0.f;
  for (int l = a.n_layers - 1; l >= 0; --l) {  // likelihood direction
    __syncthreads();  // every wave is done with the previous layer (and the image is zero-padded)
    const float* lp = layers + (int64_t)l * layer_stride;
    for (int k = tid; k < layer_stride; k += kBlock) sW[sDst[k] & 0xFFFFu] = lp[k];
    nv_stage_mask<true>(sW, a, l, d);
    __syncthreads();
    const float m = sW[M::MASK + 4 * ln.g], keep = 1.f - m;
    const float sf = expf(sW[M::SF + 4 * ln.g]);
    float xm[3][kNvT];
#pragma unroll
    for (int s = 0; s < 3; ++s)
#pragma unroll
      for (int u = 0; u < kNvT; ++u) xm[s][u] = xs[s][u] * m;
    NvV3 so, to;
    nv_mlp_fwd3(sW + M::SNET, ln, temb, xm, so);
    nv_mlp_fwd3(sW + M::TNET, ln, temb, xm, to);
#pragma unroll
    for (int u = 0; u < kNvT; ++u)  // register 0: the lane group's coordinate
      NVP_COUPLE3(tt[u], hard, sf, keep, so[0][u][0], so[1][u][0], so[2][u][0], to[0][u][0], to[1][u][0], to[2][u][0],
                  xs[0][u], xs[1][u], xs[2][u], ldj[0][u], ldj[1][u], ldj[2][u]);
  }
  // ---- base density: every lane gathers its sample's coordinates (lane 16 c + s holds coordinate c) ----
#pragma unroll
  for (int u = 0; u < kNvT; ++u) {
    float xc[3][4], lj[3];
#pragma unroll
    for (int s = 0; s < 3; ++s) {
#pragma unroll
      for (int c = 0; c < 4; ++c) xc[s][c] = __shfl(xs[s][u], 16 * c + ln.s, 64);
      float v = ldj[s][u];
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 32, 64);
      lj[s] = v;
    }
    if (ln.g == 0 && idx[u] >= 0) NVP_BASE_STORE3(a, xc, 4, d, lj, idx[u], logp, ds);
  }
}

// ---------------------------------------------------------------------------------------------
// The flow as a map on the matrix cores (pdeinv_realnvp_map's matrix-core path; celu / elu, either layout): the
// likelihood pass of realnvp_grad_kernel run in either direction, and nothing else of that kernel. 16-sample tiles
// in the v_mfma_f32_16x16x4_f32 accumulator layout, the layer image NvM<PK> staged through the nv_layer_dst table
// (the next layer's parameters in registers under this layer's math; no transposed copies), both nets through
// nv_mlp_fwd<PK>, the coupling update on the lanes that own coordinates, on the hardware exp2 / rcp as in the
// gradient kernel. A wave carries kNvT tiles through each staged layer, like its siblings.
//   REV = 1: staging order L-1 .. 0, x <- (x + tr) e^s,  ldj += sum s, logp = log p0(y) + ldj
//   REV = 0: staging order 0 .. L-1, x <- x e^{-s} - tr, ldj -= sum s, logp = log p0(x_in) - ldj
// Base form: every lane gathers its sample's coordinates from the owning lanes (__shfl), as the time kernel does.
// Stores: the owning lanes write y (packed: lane group c coordinate c; identity: lane group q coordinates
// 4q .. 4q + 3, one float4 where y_vec says that rows and pointer are 16-byte aligned), lane group 0 ldj and logp.
// Plain stores, no atomics; a sample's outputs depend on its own column of the tiles only. y may be xv (in place).
// ---------------------------------------------------------------------------------------------
constexpr int kNvWavesMapPk = 4;  // waves per SIMD, packed layout
constexpr int kNvWavesMap = 3;    // waves per SIMD, identity layout (at 4 it spills)

template <bool PK, int REV>
__global__ __launch_bounds__(kBlock, PK ? kNvWavesMapPk : kNvWavesMap) void realnvp_map_mfma_kernel(
    NvpArgs a, int d, const float* __restrict__ params, const float* __restrict__ tv, int64_t t_stride,
    const float* xv, int64_t n, int64_t ld, int64_t layer_stride, float* y, int64_t ld_y, int y_vec,
    float* __restrict__ ldj_out, float* __restrict__ logp_out) {
  using M = NvM<PK>;
  constexpr int NC = PK ? 1 : 4;    // registers that hold coordinates
  constexpr int DMAX = PK ? 4 : 8;  // coordinates a layout can hold
  __shared__ float sW[M::LAYER];    // current coupling layer (padded); the time embedding before the first
  __shared__ float sF[48];          // sinusoid table: frequency, sin weight, cos weight
  __shared__ uint32_t sDst[kNvRaw];
  const int E = a.E, n_t = a.in_dim - d, L = a.n_layers;
  const float* layers = params + nvp_temb_params(E);
  const bool hard = !a.ignore_time && a.soft_init == 0.f;
  const int tid = threadIdx.x, wave = tid >> 6;
  const NvLane ln = nv_lane(tid, false);
  nv_stage_sinusoid(sF, E, [E](int q) {  // fp32 on the device, as the gradient kernel
    const int half = E / 2;
    const float step = logf(10000.f) / (float)(half - 1);
    return expf(-step * (float)(q < half ? q : q - half));
  });
  nv_stage_init<PK>(sDst, sW, layer_stride, d, n_t);
  float pre[kNvPre];
  nv_prefetch(pre, layers, REV ? L - 1 : 0, layer_stride);
  __syncthreads();  // sW zeroed
  if (E > 0) nv_stage_temb<PK>(sW, params, E, false);
  __syncthreads();
  // base quadratic form of the sample in lane column s: (x - mean)^T inv_cov (x - mean), in every lane
  auto base_quad = [&](const f32x4& xu) {
    float xc[DMAX];
#pragma unroll
    for (int k = 0; k < DMAX; ++k) {
      const float v = __shfl(PK ? xu[0] : xu[k & 3], 16 * (PK ? k : k >> 2) + ln.s, 64);
      xc[k] = k < d ? v - a.mean[k] : 0.f;
    }
    float quad = 0.f;
#pragma unroll
    for (int r = 0; r < DMAX; ++r) {
      if (r < d) {
        float acc = 0.f;
#pragma unroll
        for (int c = 0; c < DMAX; ++c)
          if (c < d) acc = fmaf(a.inv_cov[r * d + c], xc[c], acc);
        quad = fmaf(xc[r], acc, quad);
      }
    }
    return quad;
  };
  // ---- the wave's tiles ----
  NvV x, temb;
  float tt[kNvT], ldj[kNvT], quad[kNvT];  // quad: the base form of the input (REV = 0)
  const int64_t base = (int64_t)blockIdx.x * kNvSPB + wave * 16 * kNvT;
#pragma unroll
  for (int u = 0; u < kNvT; ++u) {
    const int64_t i = base + 16 * u + ln.s;
    const bool active = i < n;
    tt[u] = active ? tv[i * t_stride] : 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int k = nv_xinv<PK>(4 * ln.g + c, d);
      x[u][c] = (active && k >= 0 && (!PK || c == 0)) ? xv[i * ld + k] : 0.f;  // packed: registers 1..3 are 0
    }
    ldj[u] = 0.f;
    quad[u] = (!REV && logp_out) ? base_quad(x[u]) : 0.f;
  }
  if (E > 0) {  // TimeEmbedding (:8-22)
    NvV se, he;
#pragma unroll
    for (int u = 0; u < kNvT; ++u)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int q = 4 * ln.g + c;
        const float e = tt[u] * sF[q];
        se[u][c] = sF[16 + q] * sinf(e) + sF[32 + q] * cosf(e);
      }
    nv_bcast(he, nv_vec(sW + M::E_B1, ln));
    nv_fwdT(sW + M::E_W1, ln, se, he);
#pragma unroll
    for (int u = 0; u < kNvT; ++u) he[u] = nv_celu4(he[u]);
    nv_bcast(temb, nv_vec(sW + M::E_B2, ln));
    nv_fwdT(sW + M::E_W2, ln, he, temb);
    __syncthreads();  // every wave has read the time embedding: back to the zero-padded layer image
    for (int q = tid; q < M::TEMB; q += kBlock) sW[q] = 0.f;
  } else {
#pragma unroll
    for (int u = 0; u < kNvT; ++u)
#pragma unroll
      for (int c = 0; c < 4; ++c) temb[u][c] = (!a.ignore_time && 4 * ln.g + c == nv_tpos<PK>(0)) ? tt[u] : 0.f;
  }
  for (int j = 0; j < L; ++j) {
    const int l = REV ? L - 1 - j : j;
    __syncthreads();  // every wave is done with the previous layer (and the image is zero-padded)
    nv_stage_mask<PK>(sW, a, l, d);
    nv_scatter_layer<false>(sW, sDst, pre, layer_stride);
    if (j + 1 < L) nv_prefetch(pre, layers, REV ? l - 1 : l + 1, layer_stride);
    __syncthreads();
    const f32x4 m = nv_vec(sW + M::MASK, ln);
    const f32x4 sfw = nv_vec(sW + M::SF, ln);
    f32x4 sf, isf;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      sf[c] = nv_exp(sfw[c]);
      isf[c] = __builtin_amdgcn_rcpf(sf[c]);
    }
    NvV xm, so, to;
    nv_masked<PK>(x, m, xm);
    {
      NvAct h;
      nv_mlp_fwd<PK>(sW + M::SNET, ln, temb, xm, h, so);
      nv_mlp_fwd<PK>(sW + M::TNET, ln, temb, xm, h, to);
    }
#pragma unroll
    for (int u = 0; u < kNvT; ++u) {
#pragma unroll
      for (int c = 0; c < NC; ++c) {  // padded / masked coordinates: keep = 0, x unchanged
        const float keep = 1.f - m[c];
        const float th = hard ? tt[u] : 1.f;
        const float sk = nv_tanh(th * so[u][c] * isf[c]) * sf[c] * keep;
        const float tr = th * to[u][c] * keep;
        if (REV) {
          x[u][c] = (x[u][c] + tr) * nv_exp(sk);
          ldj[u] += sk;
        } else {
          x[u][c] = x[u][c] * nv_exp(-sk) - tr;
          ldj[u] -= sk;
        }
      }
    }
  }
  // ---- outputs ----
#pragma unroll
  for (int u = 0; u < kNvT; ++u) {
    const int64_t i = base + 16 * u + ln.s;
    const bool active = i < n;
    const float lj = nv_group_sum(ldj[u]);  // the four lane groups' parts
    float lp = 0.f;
    if (logp_out) lp = REV ? -0.5f * (a.log_det + base_quad(x[u])) + lj : -0.5f * (a.log_det + quad[u]) - lj;
    if (active && ln.g == 0) {
      if (ldj_out) ldj_out[i] = lj;
      if (logp_out) logp_out[i] = lp;
    }
    if (active && y) {
      float* yr = y + i * ld_y;
      if constexpr (PK) {
        if (ln.g < d) yr[ln.g] = x[u][0];
      } else {
        if (y_vec && 4 * ln.g + 3 < d) {
          *reinterpret_cast<f32x4*>(yr + 4 * ln.g) = x[u];
        } else {
#pragma unroll
          for (int c = 0; c < 4; ++c)
            if (4 * ln.g + c < d) yr[4 * ln.g + c] = x[u][c];
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// The score grad_x log p_t(x) (pdeinv_realnvp_score), reverse mode per sample.
// Likelihood pass, layers l = L-1 .. 0 (m the mask, k = 1 - m, c = t under the hard parameterisation, else 1):
//   s = tanh(c s^ / f) f k, f = e^alpha;  tau = c tau^ k;  x <- (x + tau) e^s;  ldj += sum s
// then log p = log p0(x0) + ldj and the adjoint starts as g = -Sigma^-1 (x0 - mu). Backward sweep, l = 0 .. L-1,
// with x_out the layer's output and x_in its input:
//   gs = (g x_out + 1) k;  s^bar = c gs (1 - tanh^2);  tau^bar = c g e^s k
//   g <- g e^s + m (J_s^T s^bar + J_tau^T tau^bar)[:dim]
// and after layer L-1 g is the score. Kinked activations take the derivative of the branch taken.
// Each layer's input is kept, not rebuilt by inverting the layer (x_out e^{-s} - tau loses 7 - 8 x on stiff flows):
// the likelihood pass writes the coordinates the layer changes (mask 0) into the caller's workspace, [L][D][n]
// floats (sample innermost: a wave's stores and loads are one run), and the sweep reads them back. Its nets then
// see the bits the likelihood pass saw, so s, e^s and tau are that pass's.
// General path: one thread per sample on the VALU like realnvp_time_kernel (weights at wave-uniform addresses, ACT
// a template parameter, register arrays indexed by unrolled counters only); the nets keep g' of their three hidden
// layers (from nvp_act_d2, with the value) for the transposed sweep. Accurate expf / tanhf / division in the
// coupling, NvFreq frequencies. Plain stores, no atomics: deterministic.
// ---------------------------------------------------------------------------------------------
// out = g(b + [in0 | in1] @ W), d1 = g' there: rows of in0 (N0, all), then of in1 (rows i < n1 of N1)
template <int ACT, int N0, int N1, int NO>
__device__ __forceinline__ const float* nvp_dense_d1(const float* __restrict__ W, const float (&in0)[N0],
                                                     const float (&in1)[N1], int n1, float (&out)[NO],
                                                     float (&d1)[NO]) {
  asm volatile("" ::: "memory");  // no weight fetches hoisted across dense layers (register pressure)
  const float* b = W + (N0 + n1) * NO;
#pragma unroll
  for (int o = 0; o < NO; ++o) out[o] = b[o];
#pragma unroll
  for (int i = 0; i < N0; ++i)
#pragma unroll
    for (int o = 0; o < NO; ++o) out[o] = fmaf(in0[i], W[i * NO + o], out[o]);
#pragma unroll
  for (int i = 0; i < N1; ++i) {
    if (i < n1) {
#pragma unroll
      for (int o = 0; o < NO; ++o) out[o] = fmaf(in1[i], W[(N0 + i) * NO + o], out[o]);
    }
  }
#pragma unroll
  for (int o = 0; o < NO; ++o) {
    float g, g1, g2;
    nvp_act_d2<ACT>(out[o], g, g1, g2);
    out[o] = g;
    d1[o] = g1;
  }
  return b + NO;
}

// BasicMLP over [xm (D) | temb (n_t)]: its output and g' of the three hidden layers
template <int D, int ACT>
__device__ __forceinline__ const float* nvp_mlp_d1(const float* p, const float (&xm)[D], const float (&temb)[16],
                                                   int n_t, float (&out)[D], float (&a0)[8], float (&a1)[16],
                                                   float (&a2)[16]) {
  float h0[8], h1[16], h2[16];
  const float none[1] = {0.f};
  p = nvp_dense_d1<ACT, D, 16, 8>(p, xm, temb, n_t, h0, a0);
  p = nvp_dense_d1<ACT, 8, 1, 16>(p, h0, none, 0, h1, a1);
  p = nvp_dense_d1<ACT, 16, 1, 16>(p, h1, none, 0, h2, a2);
  asm volatile("" ::: "memory");
  const float* b = p + 16 * D;
#pragma unroll
  for (int k = 0; k < D; ++k) out[k] = b[k];
#pragma unroll
  for (int i = 0; i < 16; ++i)
#pragma unroll
    for (int k = 0; k < D; ++k) out[k] = fmaf(h2[i], p[i * D + k], out[k]);
  return b + D;
}

// gin += (d out / d xm)^T dout of the BasicMLP at p (n_in = D + n_t input rows), from the g' nvp_mlp_d1 kept
template <int D>
__device__ __forceinline__ void nvp_mlp_bwd_x(const float* p, int n_in, const float (&dout)[D], const float (&a0)[8],
                                              const float (&a1)[16], const float (&a2)[16], float (&gin)[D]) {
  const float* W0 = p;
  const float* W1 = W0 + n_in * 8 + 8;
  const float* W2 = W1 + 8 * 16 + 16;
  const float* W3 = W2 + 16 * 16 + 16;
  float d2[16], d1[16], d0[8];
  asm volatile("" ::: "memory");
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < D; ++k) acc = fmaf(W3[i * D + k], dout[k], acc);
    d2[i] = acc * a2[i];
  }
  asm volatile("" ::: "memory");
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    float acc = 0.f;
#pragma unroll
    for (int o = 0; o < 16; ++o) acc = fmaf(W2[i * 16 + o], d2[o], acc);
    d1[i] = acc * a1[i];
  }
  asm volatile("" ::: "memory");
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    float acc = 0.f;
#pragma unroll
    for (int o = 0; o < 16; ++o) acc = fmaf(W1[i * 16 + o], d1[o], acc);
    d0[i] = acc * a0[i];
  }
  asm volatile("" ::: "memory");
#pragma unroll
  for (int k = 0; k < D; ++k) {
    float acc = gin[k];
#pragma unroll
    for (int o = 0; o < 8; ++o) acc = fmaf(W0[k * 8 + o], d0[o], acc);
    gin[k] = acc;
  }
}

// One coordinate's coupling terms, the value stream of NVP_COUPLE3: th = tanh(c s^ / f), sk = th f k, es = e^{sk},
// tk = c tau^ k; both passes of the score kernel go through here, so the sweep's are the likelihood pass's bits.
__device__ __forceinline__ void nvp_couple1(float t, bool hard, float sf, float keep, float s, float tr, float& th,
                                            float& sk, float& es, float& tk) {
  if (hard) {
    s *= t;
    tr *= t;
  }
  th = tanhf(s / sf);
  sk = th * sf * keep;
  es = expf(sk);
  tk = tr * keep;
}

// score rows [n, D] at stride ld_s (nullable: log p only, no workspace traffic), logp nullable; ws: [L][D][n] floats.
template <int D, int ACT>
__global__ __launch_bounds__(kBlock, 2) void realnvp_score_kernel(NvpArgs a, NvFreq fr, const float* __restrict__ params,
                                                               const float* __restrict__ tv, int64_t t_stride,
                                                               const float* __restrict__ xv, int64_t n, int64_t ld,
                                                               int64_t layer_stride, float* __restrict__ score,
                                                               int64_t ld_s, float* __restrict__ logp,
                                                               float* __restrict__ ws) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const float t = tv[i * t_stride];
  float x[D];
#pragma unroll
  for (int k = 0; k < D; ++k) x[k] = xv[i * ld + k];
  float temb[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) temb[q] = 0.f;
  const float* p = params;
  const int E = a.E;
  if (!a.ignore_time) {
    if (E > 0) {
      const int half = E / 2;
      float se[16], h[16];
#pragma unroll
      for (int q = 0; q < 16; ++q) {  // position q: sin of frequency q (q < half), cos of frequency q - half
        se[q] = 0.f;
        if (q < E) {
          float sn, cs;
          sincosf(t * fr.w[q], &sn, &cs);
          se[q] = q < half ? sn : cs;
        }
      }
      // two E x E dense layers, unrolled to 16 x 16 with the rows and columns >= E skipped
      auto layer = [&](const float* W, const float (&in)[16], float (&out)[16]) {
#pragma unroll
        for (int o = 0; o < 16; ++o) out[o] = o < E ? W[E * E + o] : 0.f;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          if (q < E) {
#pragma unroll
            for (int o = 0; o < 16; ++o)
              if (o < E) out[o] = fmaf(in[q], W[q * E + o], out[o]);
          }
        }
      };
      layer(p, se, h);
#pragma unroll
      for (int o = 0; o < 16; ++o) {
        if (o < E) {
          float g, g1, g2;
          nvp_act_d2<ACT>(h[o], g, g1, g2);
          h[o] = g;
        }
      }
      p += E * E + E;
      layer(p, h, temb);
      p += E * E + E;
    } else {
      temb[0] = t;
    }
  }
  const float* layers = p;
  const bool hard = !a.ignore_time && a.soft_init == 0.f;
  const int n_t = a.in_dim - D;
  float ldj = 0.f;
  for (int l = a.n_layers - 1; l >= 0; --l) {  // likelihood direction: reversed layers
    const float* lp = layers + (int64_t)l * layer_stride;
    const float* m = a.masks + l * D;
    float xm[D];
#pragma unroll
    for (int k = 0; k < D; ++k) {
      xm[k] = x[k] * m[k];
      if (score && m[k] == 0.f) ws[((int64_t)l * D + k) * n + i] = x[k];  // the layer's input, where it changes
    }
    float sc[D], tr[D], a0[8], a1[16], a2[16];
    const float* q = nvp_mlp_d1<D, ACT>(lp + D, xm, temb, n_t, sc, a0, a1, a2);
    nvp_mlp_d1<D, ACT>(q, xm, temb, n_t, tr, a0, a1, a2);
#pragma unroll
    for (int k = 0; k < D; ++k) {
      float th, sk, es, tk;
      nvp_couple1(t, hard, expf(lp[k]), 1.f - m[k], sc[k], tr[k], th, sk, es, tk);
      x[k] = (x[k] + tk) * es;
      ldj += sk;
    }
  }
  // base density; its gradient -1/2 (A + A^T) (x0 - mean) (A need not be symmetric)
  float g[D];
  {
    float diff[D], quad = 0.f;
#pragma unroll
    for (int k = 0; k < D; ++k) diff[k] = x[k] - a.mean[k];
#pragma unroll
    for (int r = 0; r < D; ++r) {
      float acc = 0.f, accT = 0.f;
#pragma unroll
      for (int c = 0; c < D; ++c) {
        acc = fmaf(a.inv_cov[r * D + c], diff[c], acc);
        accT = fmaf(a.inv_cov[c * D + r], diff[c], accT);
      }
      quad = fmaf(diff[r], acc, quad);
      g[r] = -0.5f * (acc + accT);
    }
    if (logp) logp[i] = -0.5f * (a.log_det + quad) + ldj;
  }
  if (!score) return;
  for (int l = 0; l < a.n_layers; ++l) {  // backward sweep: x is layer l's output on entry, its input on exit
    const float* lp = layers + (int64_t)l * layer_stride;
    const float* m = a.masks + l * D;
    float xin[D], xm[D];
#pragma unroll
    for (int k = 0; k < D; ++k) {
      xin[k] = m[k] == 0.f ? ws[((int64_t)l * D + k) * n + i] : x[k];
      xm[k] = xin[k] * m[k];
    }
    float sc[D], tr[D], s0[8], s1[16], s2[16], t0[8], t1[16], t2[16];
    const float* q = nvp_mlp_d1<D, ACT>(lp + D, xm, temb, n_t, sc, s0, s1, s2);
    nvp_mlp_d1<D, ACT>(q, xm, temb, n_t, tr, t0, t1, t2);
    float sbar[D], tbar[D], gnet[D];
    const float c = hard ? t : 1.f;
#pragma unroll
    for (int k = 0; k < D; ++k) {
      const float keep = 1.f - m[k];
      float th, sk, es, tk;
      nvp_couple1(t, hard, expf(lp[k]), keep, sc[k], tr[k], th, sk, es, tk);
      const float gs = fmaf(g[k], x[k], 1.f) * keep;
      sbar[k] = c * gs * (1.f - th * th);
      tbar[k] = c * g[k] * es * keep;
      g[k] *= es;
      gnet[k] = 0.f;
      x[k] = xin[k];
    }
    nvp_mlp_bwd_x<D>(lp + D, a.in_dim, sbar, s0, s1, s2, gnet);
    nvp_mlp_bwd_x<D>(q, a.in_dim, tbar, t0, t1, t2, gnet);
#pragma unroll
    for (int k = 0; k < D; ++k) g[k] = fmaf(m[k], gnet[k], g[k]);
  }
#pragma unroll
  for (int k = 0; k < D; ++k) score[i * ld_s + k] = g[k];
}

// ---------------------------------------------------------------------------------------------
// The score on the matrix cores (pdeinv_realnvp_score's matrix-core path; celu / elu, either layout): the likelihood
// pass and the backward sweep of realnvp_grad_kernel on its tile machinery, without that kernel's weight-gradient
// products, accumulators, sample stage, slab, flush and reduce. Layers staged through the nv_layer_dst table with
// their transposed copies (2 L stagings: L-1 .. 0, then 0 .. L-1), nets through nv_mlp_fwd<PK>, their transposed
// sweep through nv_mlp_bwd_in<PK> (the input-gradient half of nv_mlp_bwd). The coupling terms are nvp_couple1's
// (accurate expf / tanhf / division), in both passes. Kept inputs: per layer and coordinate register the wave's
// tile as it sits in the lanes, [L][NC][tiles of 16 samples][64 lanes] floats (one 256-byte run per wave store and
// load); only the lanes whose coordinate the layer changes (mask 0) write and read. Base form and its gradient:
// every lane gathers its sample's coordinates from the owning lanes (__shfl), as the map kernel does. Stores: the
// owning lanes write the score as the map kernel writes y, lane group 0 logp. Plain stores, no atomics.
// ---------------------------------------------------------------------------------------------
constexpr int kNvWavesScorePk = 4;  // waves per SIMD, packed layout
constexpr int kNvWavesScore = 3;    // waves per SIMD, identity layout

// The input-gradient half of nv_mlp_bwd: gx += (d out / d xm)^T dout, from the forward's activations h
template <bool PK>
__device__ __forceinline__ void nv_mlp_bwd_in(const float* p, const NvLane& ln, const NvAct& h, const NvV& dout,
                                              NvV& gx) {
  const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
  NvV d, e;
  nv_bcast(e, z4);
  nv_fwdT<PK ? 0x1 : 0xF>(p + NvM<PK>::TR + NvM<PK>::W3, ln, dout, e);
#pragma unroll
  for (int u = 0; u < kNvT; ++u) d[u] = nv_dact4(e[u], h.h2[u]);
  nv_bcast(e, z4);
  nv_fwdT(p + NvM<PK>::TR + NvM<PK>::W2, ln, d, e);
#pragma unroll
  for (int u = 0; u < kNvT; ++u) d[u] = nv_dact4(e[u], h.h1[u]);
  nv_bcast(e, z4);
  nv_fwdT(p + NvM<PK>::TR + NvM<PK>::W1, ln, d, e);
#pragma unroll
  for (int u = 0; u < kNvT; ++u) {
    if constexpr (PK)  // registers 2, 3: padding units
      d[u] = f32x4{e[u][0] * nvp_celu_grad_h(h.h0[u][0]), e[u][1] * nvp_celu_grad_h(h.h0[u][1]), 0.f, 0.f};
    else
      d[u] = nv_dact4(e[u], h.h0[u]);
  }
  if constexpr (PK) {
    nv_bcast(e, z4);
    nv_fwdT<0x3>(p + NvM<PK>::TR + NvM<PK>::W0T, ln, d, e);
#pragma unroll
    for (int u = 0; u < kNvT; ++u) gx[u][0] += e[u][0];
  } else {
    nv_fwdT(p + NvM<PK>::TR + NvM<PK>::W0X, ln, d, gx);
  }
}

// ws: [L][NC][n_tiles][64] floats, n_tiles = ceil(n / 16) (pdeinv_realnvp_score_workspace_bytes)
template <bool PK>
__global__ __launch_bounds__(kBlock, PK ? kNvWavesScorePk : kNvWavesScore) void realnvp_score_mfma_kernel(
    NvpArgs a, NvFreq fr, int d, const float* __restrict__ params, const float* __restrict__ tv, int64_t t_stride,
    const float* __restrict__ xv, int64_t n, int64_t ld, int64_t layer_stride, float* __restrict__ score,
    int64_t ld_s, int s_vec, float* __restrict__ logp_out, float* __restrict__ ws, int64_t n_tiles) {
  using M = NvM<PK>;
  constexpr int NC = PK ? 1 : 4;    // registers that hold coordinates
  constexpr int DMAX = PK ? 4 : 8;  // coordinates a layout can hold
  __shared__ float sW[M::LAYER];    // current coupling layer (padded, with transposes); the time embedding before the first
  __shared__ float sF[48];          // sinusoid table: frequency, sin weight, cos weight
  __shared__ float sB[16 * 8];      // symmetrised inverse covariance: rows by position, columns by coordinate
  __shared__ uint32_t sDst[kNvRaw];
  const int E = a.E, n_t = a.in_dim - d, L = a.n_layers;
  const float* layers = params + nvp_temb_params(E);
  const bool hard = !a.ignore_time && a.soft_init == 0.f;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const NvLane ln = nv_lane(tid, false);
  nv_stage_sinusoid(sF, E, [&fr](int q) { return fr.w[q]; });
  nv_stage_init<PK>(sDst, sW, layer_stride, d, n_t);
  for (int q = tid; q < 16 * 8; q += kBlock) {
    const int r = nv_xinv<PK>(q / 8, d), c = q % 8;
    sB[q] = (r >= 0 && c < d) ? 0.5f * (a.inv_cov[r * d + c] + a.inv_cov[c * d + r]) : 0.f;
  }
  float pre[kNvPre];
  int staged = 0;  // layers staged so far
  auto stage_layer = [&](int l) {
    __syncthreads();  // every wave is done with the previous layer (and the image is zero-padded)
    nv_stage_mask<PK>(sW, a, l, d);
#pragma unroll
    for (int k = 0; k < kNvPre; ++k) {
      const int q = tid + k * kBlock;
      if (q < layer_stride) {
        const uint32_t t = sDst[q];
        sW[t & 0xFFFFu] = pre[k];
        if ((t >> 16) != 0xFFFFu) sW[t >> 16] = pre[k];
      }
    }
    ++staged;
    if (staged < 2 * L && (score || staged < L))
      nv_prefetch(pre, layers, staged < L ? L - 1 - staged : staged - L, layer_stride);
    __syncthreads();
  };
  nv_prefetch(pre, layers, L - 1, layer_stride);
  __syncthreads();  // sW zeroed
  if (E > 0) nv_stage_temb<PK>(sW, params, E, false);
  __syncthreads();
  // ---- the wave's tiles ----
  NvV x, g, temb;
  float tt[kNvT], ldj[kNvT];
  const int64_t base = (int64_t)blockIdx.x * kNvSPB + wave * 16 * kNvT;
#pragma unroll
  for (int u = 0; u < kNvT; ++u) {
    const int64_t i = base + 16 * u + ln.s;
    const bool active = i < n;
    tt[u] = active ? tv[i * t_stride] : 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int k = nv_xinv<PK>(4 * ln.g + c, d);
      x[u][c] = (active && k >= 0 && (!PK || c == 0)) ? xv[i * ld + k] : 0.f;  // packed: registers 1..3 are 0
    }
    ldj[u] = 0.f;
  }
  if (E > 0) {  // TimeEmbedding (:8-22)
    NvV se, he;
#pragma unroll
    for (int u = 0; u < kNvT; ++u)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int q = 4 * ln.g + c;
        float sn, cs;
        sincosf(tt[u] * sF[q], &sn, &cs);
        se[u][c] = sF[16 + q] * sn + sF[32 + q] * cs;
      }
    nv_bcast(he, nv_vec(sW + M::E_B1, ln));
    nv_fwdT(sW + M::E_W1, ln, se, he);
#pragma unroll
    for (int u = 0; u < kNvT; ++u) he[u] = nv_celu4(he[u]);
    nv_bcast(temb, nv_vec(sW + M::E_B2, ln));
    nv_fwdT(sW + M::E_W2, ln, he, temb);
    __syncthreads();  // every wave has read the time embedding: back to the zero-padded layer image
    for (int q = tid; q < M::TEMB; q += kBlock) sW[q] = 0.f;
  } else {
#pragma unroll
    for (int u = 0; u < kNvT; ++u)
#pragma unroll
      for (int c = 0; c < 4; ++c) temb[u][c] = (!a.ignore_time && 4 * ln.g + c == nv_tpos<PK>(0)) ? tt[u] : 0.f;
  }
  // the kept-input slot of (layer l, tile u, register c) for this lane; tiles past the batch have none
  auto slot = [&](int l, int u, int c) { return (((int64_t)l * NC + c) * n_tiles + (base >> 4) + u) * 64 + lane; };
  bool tile_in[kNvT];
#pragma unroll
  for (int u = 0; u < kNvT; ++u) tile_in[u] = (base >> 4) + u < n_tiles;
  // ---- likelihood pass (layers L-1 .. 0): x <- (x + tr) e^s ----
  for (int l = L - 1; l >= 0; --l) {
    stage_layer(l);
    const f32x4 m = nv_vec(sW + M::MASK, ln);
    const f32x4 sfw = nv_vec(sW + M::SF, ln);
    NvV xm, so, to;
    nv_masked<PK>(x, m, xm);
    {
      NvAct h;
      nv_mlp_fwd<PK>(sW + M::SNET, ln, temb, xm, h, so);
      nv_mlp_fwd<PK>(sW + M::TNET, ln, temb, xm, h, to);
    }
#pragma unroll
    for (int u = 0; u < kNvT; ++u) {
#pragma unroll
      for (int c = 0; c < NC; ++c) {  // padded / masked coordinates: keep = 0, x unchanged
        if (score && tile_in[u] && m[c] == 0.f) ws[slot(l, u, c)] = x[u][c];  // the layer's input, where it changes
        float th, sk, es, tk;
        nvp_couple1(tt[u], hard, expf(sfw[c]), 1.f - m[c], so[u][c], to[u][c], th, sk, es, tk);
        x[u][c] = (x[u][c] + tk) * es;
        ldj[u] += sk;
      }
    }
  }
  // ---- base density log p0(x0) and its gradient -1/2 (A + A^T) (x0 - mean) ----
#pragma unroll
  for (int u = 0; u < kNvT; ++u) {
    float xc[DMAX];
#pragma unroll
    for (int k = 0; k < DMAX; ++k) {
      const float v = __shfl(PK ? x[u][0] : x[u][k & 3], 16 * (PK ? k : k >> 2) + ln.s, 64);
      xc[k] = k < d ? v - a.mean[k] : 0.f;
    }
    float quad = 0.f;
#pragma unroll
    for (int r = 0; r < DMAX; ++r) {
      if (r < d) {
        float acc = 0.f;
#pragma unroll
        for (int c = 0; c < DMAX; ++c)
          if (c < d) acc = fmaf(a.inv_cov[r * d + c], xc[c], acc);
        quad = fmaf(xc[r], acc, quad);
      }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float acc = 0.f;
      if (!PK || c == 0) {
#pragma unroll
        for (int q = 0; q < DMAX; ++q) acc = fmaf(sB[(4 * ln.g + c) * 8 + q], xc[q], acc);
      }
      g[u][c] = -acc;
    }
    const float lj = nv_group_sum(ldj[u]);  // the four lane groups' parts
    const int64_t i = base + 16 * u + ln.s;
    if (logp_out && i < n && ln.g == 0) logp_out[i] = -0.5f * (a.log_det + quad) + lj;
  }
  if (!score) return;  // block-uniform
  // ---- backward sweep (layers 0 .. L-1): x is the layer's output on entry, its kept input on exit ----
  for (int l = 0; l < L; ++l) {
    stage_layer(l);
    const f32x4 m = nv_vec(sW + M::MASK, ln);
    const f32x4 sfw = nv_vec(sW + M::SF, ln);
    NvV xin, xm, out, es, gso, gto, gacc;
#pragma unroll
    for (int u = 0; u < kNvT; ++u) {
      xin[u] = x[u];
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (tile_in[u] && m[c] == 0.f) xin[u][c] = ws[slot(l, u, c)];
    }
    nv_masked<PK>(xin, m, xm);
    NvAct h;
    nv_mlp_fwd<PK>(sW + M::SNET, ln, temb, xm, h, out);
#pragma unroll
    for (int u = 0; u < kNvT; ++u) {
      gso[u] = gto[u] = gacc[u] = es[u] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const float keep = 1.f - m[c];
        float th, sk, ek, tk;
        nvp_couple1(tt[u], hard, expf(sfw[c]), keep, out[u][c], 0.f, th, sk, ek, tk);
        const float cc = hard ? tt[u] : 1.f;
        const float gs = fmaf(g[u][c], x[u][c], 1.f) * keep;
        es[u][c] = ek;
        gso[u][c] = cc * gs * (1.f - th * th);
        gto[u][c] = cc * g[u][c] * ek * keep;
      }
    }
    nv_mlp_bwd_in<PK>(sW + M::SNET, ln, h, gso, gacc);
    nv_mlp_fwd<PK>(sW + M::TNET, ln, temb, xm, h, out);
    nv_mlp_bwd_in<PK>(sW + M::TNET, ln, h, gto, gacc);
#pragma unroll
    for (int u = 0; u < kNvT; ++u) {
#pragma unroll
      for (int c = 0; c < NC; ++c) g[u][c] = fmaf(m[c], gacc[u][c], g[u][c] * es[u][c]);
      x[u] = xin[u];
    }
  }
  // ---- the score, from the owning lanes ----
#pragma unroll
  for (int u = 0; u < kNvT; ++u) {
    const int64_t i = base + 16 * u + ln.s;
    if (i < n) {
      float* sr = score + i * ld_s;
      if constexpr (PK) {
        if (ln.g < d) sr[ln.g] = g[u][0];
      } else {
        if (s_vec && 4 * ln.g + 3 < d) {
          *reinterpret_cast<f32x4*>(sr + 4 * ln.g) = g[u];
        } else {
#pragma unroll
          for (int c = 0; c < 4; ++c)
            if (4 * ln.g + c < d) sr[4 * ln.g + c] = g[u][c];
        }
      }
    }
  }
}

static int64_t layer_params(int D, int in_dim) {
  const int64_t mlp = (int64_t)in_dim * 8 + 8 + 8 * 16 + 16 + 16 * 16 + 16 + 16 * D + D;
  return D + 2 * mlp;
}

static int in_dim_of(const pdeinv_realnvp_desc* d) {
  return d->ignore_time ? d->dim : d->dim + (d->embed_time_dim > 0 ? d->embed_time_dim : 1);
}

// The descriptor checks of every entry point, in one fixed order; who is the entry point's message prefix (a
// literal: no string is built unless a check fails). The trailing arguments, if any, are the entry point's own
// requirement on the descriptor, checked where it always was: after the activation's range, before the host arrays.
// It is passed as one whole PDEINV_REQUIRE(...) statement: commas inside its parentheses are safe, a comma outside
// any parentheses would split it. Without it the expansion holds one empty statement.
#define NVP_REQUIRE_DESC(d, who, ...)                                                                              \
  PDEINV_REQUIRE((d) != nullptr, PDEINV_ERR_INVALID, who ": null descriptor");                                     \
  PDEINV_REQUIRE((d)->dim >= 1 && (d)->dim <= 8, PDEINV_ERR_UNSUPPORTED, who ": dim must be in [1, 8]");           \
  PDEINV_REQUIRE((d)->n_layers >= 1 && (d)->n_layers <= PDEINV_REALNVP_MAX_LAYERS, PDEINV_ERR_UNSUPPORTED,         \
                 who ": 1 <= n_layers <= 64");                                                                     \
  PDEINV_REQUIRE((d)->embed_time_dim >= 0 && (d)->embed_time_dim <= 16 && (d)->embed_time_dim % 2 == 0 &&          \
                     (d)->embed_time_dim != 2,                                                                     \
                 PDEINV_ERR_UNSUPPORTED, who ": embed_time_dim must be 0 or even in [4, 16]");                     \
  PDEINV_REQUIRE((d)->activation >= PDEINV_ACT_CELU && (d)->activation <= PDEINV_ACT_GELU, PDEINV_ERR_UNSUPPORTED, \
                 who ": unknown activation");                                                                      \
  __VA_ARGS__;                                                                                                     \
  PDEINV_REQUIRE((d)->masks && (d)->base_mean && (d)->base_inv_cov, PDEINV_ERR_INVALID, who ": null host array")

// The kernels' view of a checked descriptor
static NvpArgs nvp_args(const pdeinv_realnvp_desc* d) {
  const int D = d->dim;
  NvpArgs a{};
  a.n_layers = d->n_layers;
  a.ignore_time = d->ignore_time ? 1 : 0;
  a.E = a.ignore_time ? 0 : d->embed_time_dim;
  a.in_dim = in_dim_of(d);
  a.act = d->activation;
  a.soft_init = d->soft_init;
  a.log_det = d->base_log_det;
  for (int k = 0; k < D; ++k) a.mean[k] = d->base_mean[k];
  for (int k = 0; k < D * D; ++k) a.inv_cov[k] = d->base_inv_cov[k];
  for (int k = 0; k < d->n_layers * D; ++k) a.masks[k] = d->masks[k];
  return a;
}

// Launch of a general-path kernel K<D, ACT> (block kBlock, grid g, stream st, then K's arguments): one instantiation
// per (dim 1 .. 8, activation); celu and elu (alpha = 1) are the same map.
#define NVP_DIMS_(K, AA, D, g, st, ...)                                                     \
  switch (D) {                                                                              \
    case 1: hipLaunchKernelGGL((K<1, AA>), g, dim3(kBlock), 0, st, __VA_ARGS__); break;     \
    case 2: hipLaunchKernelGGL((K<2, AA>), g, dim3(kBlock), 0, st, __VA_ARGS__); break;     \
    case 3: hipLaunchKernelGGL((K<3, AA>), g, dim3(kBlock), 0, st, __VA_ARGS__); break;     \
    case 4: hipLaunchKernelGGL((K<4, AA>), g, dim3(kBlock), 0, st, __VA_ARGS__); break;     \
    case 5: hipLaunchKernelGGL((K<5, AA>), g, dim3(kBlock), 0, st, __VA_ARGS__); break;     \
    case 6: hipLaunchKernelGGL((K<6, AA>), g, dim3(kBlock), 0, st, __VA_ARGS__); break;     \
    case 7: hipLaunchKernelGGL((K<7, AA>), g, dim3(kBlock), 0, st, __VA_ARGS__); break;     \
    case 8: hipLaunchKernelGGL((K<8, AA>), g, dim3(kBlock), 0, st, __VA_ARGS__); break;     \
  }
#define NVP_LAUNCH_DIM_ACT(K, D, act, g, st, ...)                                                        \
  switch (act) {                                                                                         \
    case PDEINV_ACT_CELU: case PDEINV_ACT_ELU: NVP_DIMS_(K, PDEINV_ACT_CELU, D, g, st, __VA_ARGS__) break; \
    case PDEINV_ACT_RELU: NVP_DIMS_(K, PDEINV_ACT_RELU, D, g, st, __VA_ARGS__) break;                    \
    case PDEINV_ACT_TANH: NVP_DIMS_(K, PDEINV_ACT_TANH, D, g, st, __VA_ARGS__) break;                    \
    case PDEINV_ACT_SILU: NVP_DIMS_(K, PDEINV_ACT_SILU, D, g, st, __VA_ARGS__) break;                    \
    case PDEINV_ACT_SOFTPLUS: NVP_DIMS_(K, PDEINV_ACT_SOFTPLUS, D, g, st, __VA_ARGS__) break;            \
    default: NVP_DIMS_(K, PDEINV_ACT_GELU, D, g, st, __VA_ARGS__) break;                                 \
  }

// The embedding's frequencies by position (NvFreq)
static NvFreq nvp_freq(const NvpArgs& a) {
  NvFreq fr{};
  for (int q = 0; q < a.E; ++q)
    fr.w[q] = (float)exp(-(log(10000.0) / (double)(a.E / 2 - 1)) * (double)(q % (a.E / 2)));
  return fr;
}

}  // namespace pdeinv

using namespace pdeinv;

extern "C" int64_t pdeinv_realnvp_param_count(const pdeinv_realnvp_desc* d) {
  if (!d || d->dim < 1 || d->dim > 8 || d->n_layers < 1 || d->embed_time_dim < 0) return -1;
  return nvp_temb_params(d->ignore_time ? 0 : d->embed_time_dim) +
         (int64_t)d->n_layers * layer_params(d->dim, in_dim_of(d));
}

extern "C" int pdeinv_realnvp_logdensity(const pdeinv_realnvp_desc* d, const float* params, const float* t,
                                         int64_t t_stride, const float* x, int64_t n, int64_t ld, float* out,
                                         void* stream) {
  NVP_REQUIRE_DESC(d, "realnvp");
  PDEINV_REQUIRE(n >= 0 && ld >= d->dim && t_stride >= 0, PDEINV_ERR_INVALID, "realnvp: bad sizes");
  if (n == 0) return PDEINV_OK;
  PDEINV_REQUIRE(params && t && x && out, PDEINV_ERR_INVALID, "realnvp: null device pointer");
  const int D = d->dim;
  const NvpArgs a = nvp_args(d);
  const int64_t ls = layer_params(D, a.in_dim);
  hipStream_t st = (hipStream_t)stream;
  const dim3 g(grid_for(n));
  switch (D) {
#define CASE(DD) case DD: hipLaunchKernelGGL(realnvp_logdensity_kernel<DD>, g, dim3(kBlock), 0, st, a, params, t, t_stride, x, n, ld, ls, out); break;
    CASE(1) CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8)
#undef CASE
  }
  return check_launch("realnvp_logdensity_kernel");
}

// Packed layout where [x | temb] fits one 16-vector with x in register 0; the identity layout otherwise (d > 4)
static bool nvp_packed(const pdeinv_realnvp_desc* d) { return d->dim <= 4 && in_dim_of(d) - d->dim <= 12; }
static NvSlabMap nvp_slab_map(const pdeinv_realnvp_desc* d) {
  NvSlabMap m{};
  m.d = d->dim;
  m.n_t = in_dim_of(d) - d->dim;
  m.pk = nvp_packed(d) ? 1 : 0;
  m.n_layers = d->n_layers;
  m.layer_stride = layer_params(d->dim, in_dim_of(d));
  m.temb_params = nvp_temb_params(d->ignore_time ? 0 : d->embed_time_dim);
  m.n_params = m.temb_params + (int64_t)d->n_layers * m.layer_stride;
  m.cb = m.pk ? NvC<true>::LAYER : NvC<false>::LAYER;
  return m;
}

static int64_t nvp_grad_rows(int64_t n) {
  const int64_t tiles = (n + kNvSPB - 1) / kNvSPB;
  return tiles < kNvpMaxRows ? tiles : kNvpMaxRows;
}

extern "C" int64_t pdeinv_realnvp_grad_workspace(const pdeinv_realnvp_desc* d, int64_t n) {
  const int64_t P = pdeinv_realnvp_param_count(d);
  if (P < 0 || n < 0) return -1;
  const int64_t slab = nvp_grad_rows(n) * nv_slab_ld(nvp_slab_map(d)) * (int64_t)sizeof(float);
  return slab + (1 + kNvSplits) * (P + 1) * (int64_t)sizeof(double);
}
extern "C" int pdeinv_realnvp_value_and_grad(const pdeinv_realnvp_desc* d, const float* params, const float* t,
                                             int64_t t_stride, const float* x, int64_t n, int64_t ld, float* loss,
                                             float* grad, void* workspace, int64_t workspace_bytes, void* stream) {
  NVP_REQUIRE_DESC(
      d, "realnvp",
      PDEINV_REQUIRE(d->activation == PDEINV_ACT_CELU || d->activation == PDEINV_ACT_ELU, PDEINV_ERR_UNSUPPORTED,
                     "realnvp: value_and_grad is built for celu / elu (the flow of log_density_estimation.py:103-114)"));
  PDEINV_REQUIRE(n >= 1 && ld >= d->dim && t_stride >= 0, PDEINV_ERR_INVALID,
                 "realnvp: value_and_grad needs n >= 1 rows (the loss is a mean)");
  PDEINV_REQUIRE(params && t && x && loss && grad && workspace, PDEINV_ERR_INVALID, "realnvp: null device pointer");
  PDEINV_REQUIRE(workspace_bytes >= pdeinv_realnvp_grad_workspace(d, n), PDEINV_ERR_INVALID,
                 "realnvp: workspace too small (pdeinv_realnvp_grad_workspace)");
  const int D = d->dim;
  const NvpArgs a = nvp_args(d);
  const int64_t ls = layer_params(D, a.in_dim);
  const int64_t P = pdeinv_realnvp_param_count(d);
  const int64_t rows_max = nvp_grad_rows(n);
  const NvSlabMap map = nvp_slab_map(d);
  const int64_t sld = nv_slab_ld(map);
  float* slab = (float*)workspace;
  double* acc64 = (double*)((char*)workspace + rows_max * sld * (int64_t)sizeof(float));
  double* parts = acc64 + (P + 1);
  hipStream_t st = (hipStream_t)stream;
  const int64_t tiles = (n + kNvSPB - 1) / kNvSPB;
  // any d <= 8 (padded coordinates stay fixed); celu and elu are the same map.
  const bool packed = map.pk != 0;
  for (int64_t tile0 = 0; tile0 < tiles; tile0 += rows_max) {
    const int64_t rows = tiles - tile0 < rows_max ? tiles - tile0 : rows_max;
    const dim3 g((unsigned)rows);
    if (packed)
      hipLaunchKernelGGL(realnvp_grad_kernel<true>, g, dim3(kBlock), 0, st, a, D, params, t, t_stride, x, n, ld, ls,
                         P, tile0, slab, sld);
    else
      hipLaunchKernelGGL(realnvp_grad_kernel<false>, g, dim3(kBlock), 0, st, a, D, params, t, t_stride, x, n, ld, ls,
                         P, tile0, slab, sld);
    int rc = check_launch("realnvp_grad_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(nvp_slab_split_kernel, dim3((unsigned)((P + 1 + 63) / 64), kNvSplits), dim3(kBlock), 0, st,
                       slab, (int)rows, sld, map, P + 1, parts);
    rc = check_launch("nvp_slab_split_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(nvp_grad_reduce_kernel, dim3((unsigned)((P + 1 + kBlock - 1) / kBlock)), dim3(kBlock), 0, st,
                       parts, P, acc64, tile0 == 0 ? 1 : 0, tile0 + rows >= tiles ? 1 : 0, -1.0 / (double)n, grad,
                       loss);
    rc = check_launch("nvp_grad_reduce_kernel");
    if (rc) return rc;
  }
  return PDEINV_OK;
}

// Path selector of the time-derivative entry points (tests and tools/nvp_time_bench.py): 0 = AUTO, 1 = the general
// per-thread path, 2 = the matrix-core path (UNSUPPORTED outside its envelope). Process-wide.
static int g_nvp_time_impl = 0;
// The matrix-core path's envelope. AUTO takes the path wherever it applies, a choice made by measurement: it is
// faster than the general path on both batches.
static bool nvp_time_mfma_ok(const pdeinv_realnvp_desc* d) {
  return (d->activation == PDEINV_ACT_CELU || d->activation == PDEINV_ACT_ELU) && d->dim <= 4 && !d->ignore_time &&
         d->embed_time_dim >= 4 && d->embed_time_dim <= 12;
}

// Shared by the two time-derivative entry points: n_rows == 0 is the per-sample view (t_stride), n_rows > 0 the
// sets view (realnvp_time_kernel).
static int nvp_time_launch(const pdeinv_realnvp_desc* d, const float* params, const float* t, int64_t t_stride,
                           const float* x, int64_t n, int64_t ld, int64_t n_rows, int64_t set_stride, float* logp,
                           float* ds, void* stream) {
  NVP_REQUIRE_DESC(d, "realnvp_time_derivs");
  PDEINV_REQUIRE(n >= 0 && ld >= d->dim && t_stride >= 0 && set_stride >= 0, PDEINV_ERR_INVALID,
                 "realnvp_time_derivs: bad sizes");
  PDEINV_REQUIRE(n <= (int64_t)0x7FFFFFFF * kBlock, PDEINV_ERR_INVALID, "realnvp_time_derivs: too many samples");
  if (n == 0) return PDEINV_OK;
  PDEINV_REQUIRE(params && t && x && ds, PDEINV_ERR_INVALID, "realnvp_time_derivs: null device pointer");
  PDEINV_REQUIRE(((uintptr_t)ds & 7) == 0 && ((uintptr_t)params & 3) == 0 && ((uintptr_t)t & 3) == 0 &&
                     ((uintptr_t)x & 3) == 0 && ((uintptr_t)logp & 3) == 0,
                 PDEINV_ERR_INVALID, "realnvp_time_derivs: misaligned pointer (d_ds needs 8 bytes, the others 4)");
  const int D = d->dim;
  const NvpArgs a = nvp_args(d);
  const NvFreq fr = nvp_freq(a);
  const int64_t ls = layer_params(D, a.in_dim);
  hipStream_t st = (hipStream_t)stream;
  PDEINV_REQUIRE(g_nvp_time_impl != 2 || nvp_time_mfma_ok(d), PDEINV_ERR_UNSUPPORTED,
                 "realnvp_time_derivs: the matrix-core path takes celu / elu, dim <= 4, 4 <= E <= 12, no ignore_time");
  if (g_nvp_time_impl != 1 && nvp_time_mfma_ok(d)) {  // forced (checked above), or AUTO inside the envelope
    hipLaunchKernelGGL(realnvp_time_mfma_kernel, dim3(grid_for(n, kNvSPB)), dim3(kBlock), 0, st, a, fr, D, params, t,
                       t_stride, x, n, ld, n_rows, set_stride, ls, logp, ds);
    return check_launch("realnvp_time_mfma_kernel");
  }
  const dim3 g(grid_for(n));
  NVP_LAUNCH_DIM_ACT(realnvp_time_kernel, D, a.act, g, st, a, fr, params, t, t_stride, x, n, ld, n_rows, set_stride, ls, logp,
                     ds);
  return check_launch("realnvp_time_kernel");
}

extern "C" int pdeinv_realnvp_time_derivs(const pdeinv_realnvp_desc* d, const float* params, const float* t,
                                          int64_t t_stride, const float* x, int64_t n, int64_t ld, float* logp,
                                          float* ds, void* stream) {
  return nvp_time_launch(d, params, t, t_stride, x, n, ld, 0, 0, logp, ds, stream);
}

extern "C" int pdeinv_realnvp_time_derivs_sets(const pdeinv_realnvp_desc* d, const float* params, const float* tau,
                                               const float* z, int64_t n_sets, int64_t n_rows, int64_t set_stride,
                                               int64_t ld, float* logp, float* ds, void* stream) {
  PDEINV_REQUIRE(n_sets >= 0 && n_rows >= 0, PDEINV_ERR_INVALID, "realnvp_time_derivs_sets: negative sizes");
  PDEINV_REQUIRE(n_sets == 0 || n_rows <= INT64_MAX / n_sets, PDEINV_ERR_INVALID,
                 "realnvp_time_derivs_sets: n_sets * n_rows overflows");
  if (d && ld == 0) ld = 2 * (int64_t)d->dim;  // rows [x | v], as pdeinv_kmv_weights
  return nvp_time_launch(d, params, tau, 1, z, n_sets * n_rows, ld, n_rows, set_stride, logp, ds, stream);
}

extern "C" int pdeinv_realnvp_time_impl(const pdeinv_realnvp_desc* d, int32_t impl) {
  if (impl >= 0 && impl <= 2) g_nvp_time_impl = impl;
  if (!d) return g_nvp_time_impl;
  if (g_nvp_time_impl == 2) return nvp_time_mfma_ok(d) ? 1 : PDEINV_ERR_UNSUPPORTED;
  return g_nvp_time_impl == 0 && nvp_time_mfma_ok(d) ? 1 : 0;
}

// ---- the flow as a map (pdeinv_realnvp_map) and the score (pdeinv_realnvp_score): the path ----
// The envelope of both matrix-core paths: that of pdeinv_realnvp_value_and_grad (celu / elu; any dim <= 8, any E,
// ignore_time; packed layout where nvp_packed holds, identity layout otherwise). It is also AUTO's rule, a choice made
// by measurement: the matrix-core path was faster than the general one on every batch of every descriptor class in
// the envelope (the map: DESIGN.md §4.2.2; the score: §4.2.3, tools/nvp_score_bench.py, 2.2 - 4.9 x).
static bool nvp_tile_ok(const pdeinv_realnvp_desc* d) {
  return d->activation == PDEINV_ACT_CELU || d->activation == PDEINV_ACT_ELU;
}

// The descriptor and impl checks of an entry point of either, then path: 0 general, 1 matrix-core (who: the entry
// point's message prefix)
#define NVP_IMPL_PATH(d, impl, who, path)                                                                    \
  NVP_REQUIRE_DESC(d, who);                                                                                  \
  PDEINV_REQUIRE((impl) == PDEINV_NVP_TIME_AUTO || (impl) == PDEINV_NVP_TIME_GENERAL ||                      \
                     (impl) == PDEINV_NVP_TIME_MATRIX,                                                       \
                 PDEINV_ERR_INVALID, who ": impl must be PDEINV_NVP_TIME_AUTO, _GENERAL or _MATRIX");        \
  PDEINV_REQUIRE((impl) != PDEINV_NVP_TIME_MATRIX || nvp_tile_ok(d), PDEINV_ERR_UNSUPPORTED,                 \
                 who ": the matrix-core path takes celu / elu flows");                                       \
  const int path = (impl) == PDEINV_NVP_TIME_MATRIX || ((impl) == PDEINV_NVP_TIME_AUTO && nvp_tile_ok(d)) ? 1 : 0

extern "C" int pdeinv_realnvp_map_path(const pdeinv_realnvp_desc* d, int32_t impl) {
  NVP_IMPL_PATH(d, impl, "realnvp_map_path", path);
  return path;
}

extern "C" int pdeinv_realnvp_map(const pdeinv_realnvp_desc* d, const float* params, const float* t, int64_t t_stride,
                                  const float* x, int64_t n, int64_t ld, int32_t reverse, int32_t impl, float* y,
                                  int64_t ld_y, float* ldj, float* logp, void* stream) {
  NVP_IMPL_PATH(d, impl, "realnvp_map", path);
  PDEINV_REQUIRE(reverse == 0 || reverse == 1, PDEINV_ERR_INVALID, "realnvp_map: reverse must be 0 or 1");
  if (ld_y == 0) ld_y = d->dim;
  PDEINV_REQUIRE(n >= 0 && ld >= d->dim && ld_y >= d->dim && t_stride >= 0, PDEINV_ERR_INVALID,
                 "realnvp_map: bad sizes (n >= 0, ld_x >= dim, ld_y >= dim or 0, t_stride >= 0)");
  PDEINV_REQUIRE(n <= (int64_t)0x7FFFFFFF * 128, PDEINV_ERR_INVALID, "realnvp_map: too many samples");
  PDEINV_REQUIRE((((uintptr_t)params | (uintptr_t)t | (uintptr_t)x | (uintptr_t)y | (uintptr_t)ldj | (uintptr_t)logp) & 3) == 0,
                 PDEINV_ERR_INVALID, "realnvp_map: misaligned pointer (4 bytes)");
  if (n == 0) return PDEINV_OK;
  PDEINV_REQUIRE(y || ldj || logp, PDEINV_ERR_INVALID, "realnvp_map: no output requested (d_y, d_ldj, d_logp all null)");
  PDEINV_REQUIRE(params && t && x, PDEINV_ERR_INVALID, "realnvp_map: null device pointer");
  const int D = d->dim;
  const NvpArgs a = nvp_args(d);
  const int64_t ls = layer_params(D, a.in_dim);
  hipStream_t st = (hipStream_t)stream;
  if (path == 1) {
    const dim3 g(grid_for(n, kNvSPB));
    const int y_vec = y && ld_y % 4 == 0 && ((uintptr_t)y & 15) == 0 ? 1 : 0;
#define MAPK(PKK, RR) hipLaunchKernelGGL((realnvp_map_mfma_kernel<PKK, RR>), g, dim3(kBlock), 0, st, a, D, params, t, t_stride, x, n, ld, ls, y, ld_y, y_vec, ldj, logp)
    if (nvp_packed(d)) {
      if (reverse) MAPK(true, 1); else MAPK(true, 0);
    } else {
      if (reverse) MAPK(false, 1); else MAPK(false, 0);
    }
#undef MAPK
    return check_launch("realnvp_map_mfma_kernel");
  }
  const dim3 g(grid_for(n));
#define CASE(DD, RR) case DD: hipLaunchKernelGGL((realnvp_map_kernel<DD, RR>), g, dim3(kBlock), 0, st, a, params, t, t_stride, x, n, ld, ls, y, ld_y, ldj, logp); break;
#define DIMS(RR) switch (D) { CASE(1, RR) CASE(2, RR) CASE(3, RR) CASE(4, RR) CASE(5, RR) CASE(6, RR) CASE(7, RR) CASE(8, RR) }
  if (reverse) { DIMS(1) } else { DIMS(0) }
#undef DIMS
#undef CASE
  return check_launch("realnvp_map_kernel");
}

// ---- the score grad_x log p_t(x) (pdeinv_realnvp_score) ----
extern "C" int pdeinv_realnvp_score_path(const pdeinv_realnvp_desc* d, int32_t impl) {
  NVP_IMPL_PATH(d, impl, "realnvp_score_path", path);
  return path;
}

// The kept layer inputs. General path: [n_layers][dim][n] floats; matrix-core path: [n_layers][NC][tiles of 16
// samples][64 lanes] floats, NC = 1 coordinate register in the packed layout, 4 in the identity layout. 0 for
// arguments the entry point refuses.
extern "C" size_t pdeinv_realnvp_score_workspace_bytes(const pdeinv_realnvp_desc* d, int64_t n, int32_t impl) {
  if (!d || d->dim < 1 || d->dim > 8 || d->n_layers < 1 || d->n_layers > PDEINV_REALNVP_MAX_LAYERS || n < 0 ||
      impl < PDEINV_NVP_TIME_AUTO || impl > PDEINV_NVP_TIME_MATRIX)
    return 0;
  if (impl == PDEINV_NVP_TIME_MATRIX && !nvp_tile_ok(d)) return 0;
  if (impl == PDEINV_NVP_TIME_MATRIX || (impl == PDEINV_NVP_TIME_AUTO && nvp_tile_ok(d)))
    return (size_t)d->n_layers * (nvp_packed(d) ? 1 : 4) * (size_t)((n + 15) / 16) * 64 * sizeof(float);
  return (size_t)d->n_layers * (size_t)d->dim * (size_t)n * sizeof(float);
}

extern "C" int pdeinv_realnvp_score(const pdeinv_realnvp_desc* d, const float* params, const float* t,
                                    int64_t t_stride, const float* x, int64_t n, int64_t ld, int32_t impl,
                                    float* score, int64_t ld_s, float* logp, void* workspace, size_t workspace_bytes,
                                    void* stream) {
  NVP_IMPL_PATH(d, impl, "realnvp_score", path);
  if (ld_s == 0) ld_s = d->dim;
  PDEINV_REQUIRE(n >= 0 && ld >= d->dim && ld_s >= d->dim && t_stride >= 0, PDEINV_ERR_INVALID,
                 "realnvp_score: bad sizes (n >= 0, ld_x >= dim, ld_s >= dim or 0, t_stride >= 0)");
  PDEINV_REQUIRE(n <= (int64_t)0x7FFFFFFF * 128, PDEINV_ERR_INVALID, "realnvp_score: too many samples");
  PDEINV_REQUIRE((((uintptr_t)params | (uintptr_t)t | (uintptr_t)x | (uintptr_t)score | (uintptr_t)logp |
                   (uintptr_t)workspace) & 3) == 0,
                 PDEINV_ERR_INVALID, "realnvp_score: misaligned pointer (4 bytes)");
  if (n == 0) return PDEINV_OK;
  PDEINV_REQUIRE(score || logp, PDEINV_ERR_INVALID, "realnvp_score: no output requested (d_score, d_logp both null)");
  PDEINV_REQUIRE(params && t && x, PDEINV_ERR_INVALID, "realnvp_score: null device pointer");
  PDEINV_REQUIRE(!score || (workspace && workspace_bytes >= pdeinv_realnvp_score_workspace_bytes(d, n, impl)),
                 PDEINV_ERR_INVALID, "realnvp_score: workspace too small (pdeinv_realnvp_score_workspace_bytes)");
  const int D = d->dim;
  const NvpArgs a = nvp_args(d);
  const NvFreq fr = nvp_freq(a);
  const int64_t ls = layer_params(D, a.in_dim);
  hipStream_t st = (hipStream_t)stream;
  if (path == 1) {
    const dim3 g(grid_for(n, kNvSPB));
    const int s_vec = score && ld_s % 4 == 0 && ((uintptr_t)score & 15) == 0 ? 1 : 0;
    const int64_t n_tiles = (n + 15) / 16;
    if (nvp_packed(d))
      hipLaunchKernelGGL(realnvp_score_mfma_kernel<true>, g, dim3(kBlock), 0, st, a, fr, D, params, t, t_stride, x, n,
                         ld, ls, score, ld_s, s_vec, logp, (float*)workspace, n_tiles);
    else
      hipLaunchKernelGGL(realnvp_score_mfma_kernel<false>, g, dim3(kBlock), 0, st, a, fr, D, params, t, t_stride, x, n,
                         ld, ls, score, ld_s, s_vec, logp, (float*)workspace, n_tiles);
    return check_launch("realnvp_score_mfma_kernel");
  }
  const dim3 g(grid_for(n));
  NVP_LAUNCH_DIM_ACT(realnvp_score_kernel, D, a.act, g, st, a, fr, params, t, t_stride, x, n, ld, ls, score, ld_s, logp,
                     (float*)workspace);
  return check_launch("realnvp_score_kernel");
}
