// mlp_tile.h — the 16-row fp32-MFMA tile of the reference's narrow hypothesis nets (core/model.py:32-62:
// tanh layers, Dense(40), sum of squares; dim <= 8, width <= 20 zero-padded to 20, 1 <= n_layers <= 8, any
// out_features) and what every kernel built on it shares: the P-layout helpers, the weight image's plan and
// builder, the value / input-gradient tile body (tile_grad), the pair force (the mean over a reference set of
// grad Phi(x_i - r_j): chunk partials and their reduce) and the host side of a tile kernel (envelope, workspace
// plan, CU count, dynamic-LDS limit). tile_grad runs in the pair-force kernel (mlp_pairs_mfma.hip: pass 0 of the
// KMV residual and the learned interaction of sde_mf_mlp.hip) and in both kernels of sde_mlp.hip; pass 2 of the
// residual (kmvq_grad_kernel, mlp_pairs_mfma.hip) carries four Taylor streams through its own tile body.
//
// Layout (see mlp_pairs_mfma.hip for the full account). Every activation tile is the C/D fragment of a
// v_mfma_f32_16x16x4_f32: the row (pair / particle) on lane & 15, the feature on (lane >> 4, register) — the
// "P layout". A width-20 layer output is two 16-row M blocks whose 20 real features sit in 5 compact slots, and
// slot k is directly the B operand of k-step k of the next product: layers chain in registers. The weights are
// the A operand, lane-linear fragments of one image per call, staged into LDS by the kernel that uses them.
#pragma once
#include "common.h"

namespace pdeinv {
namespace mlpq {

constexpr int kW = 20;       // padded hidden width
constexpr int kNS = 5;       // compact slots of a hidden stream
constexpr int kLMax = 8;     // hidden (tanh) layers
constexpr int kChunk = 256;  // references per work unit of the pair force (16 tiles)

// feature carried by compact slot k in lane group g, for a stream of ns slots
__host__ __device__ inline int slot_feat(int ns, int k, int g) {
  const int fm = ns / 4;
  return k < 4 * fm ? 16 * (k >> 2) + 4 * g + (k & 3) : 16 * fm + 4 * (k - 4 * fm) + g;
}
// feature of M row r of block mb (-1: a padding row)
__host__ __device__ inline int row_feat(int ns, int mb, int r) {
  const int fm = ns / 4;
  if (mb < fm) return 16 * mb + r;
  return (r & 3) < ns % 4 ? 16 * fm + 4 * (r & 3) + (r >> 2) : -1;
}

__device__ __forceinline__ float ftanh(float z) {
  const float e = __builtin_amdgcn_exp2f(2.8853900817779268f * z);
  return 1.f - 2.f * __builtin_amdgcn_rcpf(e + 1.f);
}

__device__ __forceinline__ f32x4 mfma(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// N consecutive 64-lane units of the image starting at unit u0 (u0 % 4 == 0): 16-B reads
template <int N>
__device__ __forceinline__ void load_units(const float* img, int u0, int lane, float (&w)[N]) {
  static_assert(N % 4 == 0, "units come in fours");
  const f32x4* q = reinterpret_cast<const f32x4*>(img) + (u0 >> 2) * 64 + lane;
#pragma unroll
  for (int c = 0; c < N / 4; ++c) {
    const f32x4 v = q[c * 64];
    w[4 * c] = v[0]; w[4 * c + 1] = v[1]; w[4 * c + 2] = v[2]; w[4 * c + 3] = v[3];
  }
}

// bias-initialised accumulators of a width-20 layer (slots 0..4 -> blocks 0 / 1)
__device__ __forceinline__ void bias_hidden(const float* img, int boff, int g, f32x4 (&A)[2]) {
  const float* b = img + boff;
  A[0] = f32x4{b[4 * g], b[4 * g + 1], b[4 * g + 2], b[4 * g + 3]};
  A[1] = f32x4{b[16 + g], 0.f, 0.f, 0.f};
}
__device__ __forceinline__ void compact_hidden(const f32x4 (&A)[2], float (&z)[kNS]) {
  z[0] = A[0][0]; z[1] = A[0][1]; z[2] = A[0][2]; z[3] = A[0][3]; z[4] = A[1][0];
}

// layer-0 lane values: dimension k = 4 kk + g of the lane's group (0 past D)
template <int KD>
__device__ __forceinline__ void lane_dims(const float* row, int D, int g, float (&x)[KD]) {
#pragma unroll
  for (int kk = 0; kk < KD; ++kk) {
    const int k = 4 * kk + g;
    x[kk] = k < D ? row[k] : 0.f;
  }
}

// Reference row j of a chunk ending at j_end, coordinates 4 kk + g: an unconditional load from a clamped
// (row, coordinate), always inside r, masked after the load (0 past j_end and past D).
template <int KD>
__device__ __forceinline__ void load_ref(const float* r, int64_t ld, int D, int g, int64_t j, int64_t j_end,
                                         float (&xn)[KD]) {
#pragma unroll
  for (int kk = 0; kk < KD; ++kk) {
    const int k = 4 * kk + g;
    const float v = r[(j < j_end ? j : j_end - 1) * ld + (k < D ? k : D - 1)];
    xn[kk] = (j < j_end && k < D) ? v : 0.f;
  }
}

// -------------------------------------------------------------------------------------------------
// weight image: lane-linear A-operand fragments, unit u of a section at ((u >> 2) * 64 + lane) * 4 + (u & 3)
// -------------------------------------------------------------------------------------------------
constexpr int kMaxSec = 2 * (kLMax + 1);
struct ImageArgs {
  int L, D, W, O, KD;
  int nsec;
  int sec_layer[kMaxSec], sec_bwd[kMaxSec], sec_mb[kMaxSec], sec_u0[kMaxSec], sec_units[kMaxSec];
  int64_t roff[kLMax + 1];
  int bias_off[kLMax + 1];
  int h0_off;  // float offset of h0 (kW + 4 floats)
  int units_total, img_floats;
};

// The image's plan for a dim -> width x L -> out net: per layer the forward then the backward section (each
// rounded to 4 units), the bias slots, the h0 slot and the flat flax parameter offsets (roff).
struct ImagePlan {
  ImageArgs ia;
  int KD;
  int fwd[kLMax + 1], bwd[kLMax + 1];  // first unit of layer l's forward / backward section
};
inline ImagePlan image_plan(int dim, int L, int width, int out_features) {
  ImagePlan p{};
  p.KD = dim <= 4 ? 1 : 2;
  ImageArgs& ia = p.ia;
  ia.L = L; ia.D = dim; ia.W = width; ia.O = out_features; ia.KD = p.KD;
  // image sections: per layer forward then backward, each rounded to 4 units
  int u = 0, ns = 0;
  auto sec = [&](int l, int bwd, int ks, int mb) {
    ia.sec_layer[ns] = l; ia.sec_bwd[ns] = bwd; ia.sec_mb[ns] = mb; ia.sec_u0[ns] = u;
    ia.sec_units[ns] = ks * mb;
    ++ns;
    const int at = u;
    u += (ks * mb + 3) & ~3;
    return at;
  };
  for (int l = 0; l <= L; ++l) {
    p.fwd[l] = sec(l, 0, l == 0 ? 2 : kNS, 2);  // layer 0: KD <= 2 k-steps (zeros past KD); layer L: M
    p.bwd[l] = l < L ? sec(l, 1, kNS, l == 0 ? 1 : 2) : 0;
  }
  ia.nsec = ns;
  ia.units_total = u;
  int bf = u * 64;
  for (int l = 0; l <= L; ++l) {
    ia.bias_off[l] = bf;
    bf += kW + 4;  // layer L: c0 [20], |y0|^2
  }
  ia.h0_off = bf;
  bf += kW + 4;
  ia.img_floats = (bf + 3) & ~3;
  int64_t ro = 0;
  for (int l = 0; l <= L; ++l) {
    const int din = l == 0 ? dim : width, dout = l == L ? out_features : width;
    ia.roff[l] = ro;
    ro += (int64_t)din * dout + dout;
  }
  return p;
}

// Builds the image on the stream from the device parameter vector (flat flax order), no host copy and no
// synchronisation: kmvq_h0_kernel then kmvq_image_kernel (mlp_pairs_mfma.hip). h0y0: W + O doubles of scratch
// (h0 = the last tanh layer at input 0, y0 = K_L^T h0 + b: the expansion point of the folded output layer);
// img: ia.img_floats floats.
int build_image(const ImageArgs& ia, const float* params, double* h0y0, float* img, hipStream_t st);

// -------------------------------------------------------------------------------------------------
// value and input gradient of one 16-row tile
// -------------------------------------------------------------------------------------------------
// What a kernel needs of the image to run the tile body (kernel argument; the offsets of ImagePlan).
struct TileNet {
  int L, D;
  const float* img;  // device image (the kernel stages it into LDS)
  int img_floats;
  int fwd[kLMax + 1], bwd[kLMax + 1], bias[kLMax + 1];  // unit offsets (fwd / bwd), float offsets (bias)
  int fwd_out, bias_out, h0_off;
};
inline TileNet tile_net(const ImagePlan& p, const float* img) {
  TileNet t{};
  t.L = p.ia.L; t.D = p.ia.D; t.img = img; t.img_floats = p.ia.img_floats;
  for (int l = 0; l <= p.ia.L; ++l) {
    t.fwd[l] = p.fwd[l]; t.bwd[l] = p.bwd[l]; t.bias[l] = p.ia.bias_off[l];
  }
  t.fwd_out = p.fwd[p.ia.L];
  t.bias_out = p.ia.bias_off[p.ia.L];
  t.h0_off = p.ia.h0_off;
  return t;
}

// the block's LDS copy of the image (the caller synchronises before the first read)
__device__ __forceinline__ void stage_image(f32x4* lds4, const TileNet& net) {
  const f32x4* src = reinterpret_cast<const f32x4*>(net.img);
  for (int q = threadIdx.x; q < net.img_floats / 4; q += blockDim.x) lds4[q] = src[q];
}

// V(x) and grad V(x) of the 16 rows of a tile. img: the LDS copy of the image. x: the row's coordinates
// 4 kk + g on lane (row, g) (lane_dims; zero past D). Returns the last backward product's C fragment: register r
// of lane (row, g) is d V / d x_{4 g + r} of the row (zero past D). VALUE: `value` = V of the lane's row (the same on its four lane
// groups), from the folded output layer V = dh^T M dh + 2 c0^T dh + |y0|^2, dh = h - h0.
// `lane` must be opaque to the compiler inside a loop (asm volatile "+v"): the weight fragments are the same for
// every tile and step, and a visible lane index lets the compiler hoist all of them (hundreds of VGPRs).
template <int KD, bool VALUE>
__device__ __forceinline__ f32x4 tile_grad(const float* img, const TileNet& t, int lane, const float (&x)[KD],
                                           float& value) {
  const int gq = lane >> 4, L = t.L;
  float ckh[kLMax][kNS];  // the forward checkpoints: tanh outputs of every layer
  {
    float w0[4];
    load_units<4>(img, t.fwd[0], lane, w0);  // unit kk * 2 + mb
    f32x4 A[2];
    bias_hidden(img, t.bias[0], gq, A);
#pragma unroll
    for (int kk = 0; kk < KD; ++kk)
#pragma unroll
      for (int mb = 0; mb < 2; ++mb) A[mb] = mfma(w0[kk * 2 + mb], x[kk], A[mb]);
    float z[kNS];
    compact_hidden(A, z);
#pragma unroll
    for (int k = 0; k < kNS; ++k) ckh[0][k] = ftanh(z[k]);
  }
  float h[kNS];
#pragma unroll
  for (int k = 0; k < kNS; ++k) h[k] = ckh[0][k];
#pragma unroll
  for (int l = 1; l < kLMax; ++l) {
    if (l < L) {
      float w[12];
      load_units<12>(img, t.fwd[l], lane, w);
      f32x4 A[2];
      bias_hidden(img, t.bias[l], gq, A);
#pragma unroll
      for (int kk = 0; kk < kNS; ++kk)
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) A[mb] = mfma(w[kk * 2 + mb], h[kk], A[mb]);
      float z[kNS];
      compact_hidden(A, z);
#pragma unroll
      for (int k = 0; k < kNS; ++k) h[k] = ckh[l][k] = ftanh(z[k]);
    }
  }
  float hb[kNS];
  {  // dV/dh = 2 (M (h - h0) + c0): the output layer as a quadratic form
    const float* h0p = img + t.h0_off;
#pragma unroll
    for (int k = 0; k < 4; ++k) h[k] -= h0p[4 * gq + k];
    h[4] -= h0p[16 + gq];
    float w[12];
    load_units<12>(img, t.fwd_out, lane, w);
    f32x4 Mh[2] = {};
#pragma unroll
    for (int kk = 0; kk < kNS; ++kk)
#pragma unroll
      for (int mb = 0; mb < 2; ++mb) Mh[mb] = mfma(w[kk * 2 + mb], h[kk], Mh[mb]);
    float m[kNS];
    compact_hidden(Mh, m);
    const float* cb = img + t.bias_out;  // c0 [20], |y0|^2
    float T0 = 0.f;
#pragma unroll
    for (int k = 0; k < kNS; ++k) {
      const float c = k < 4 ? cb[4 * gq + k] : cb[16 + gq];
      const float m0 = m[k] + c;  // M dh + c0
      hb[k] = 2.f * m0;
      if constexpr (VALUE) T0 = fmaf(h[k], m0 + c, T0);
    }
    if constexpr (VALUE) {  // the row's 20 features sit on its four lane groups
      T0 += __shfl_xor(T0, 16, 64);
      T0 += __shfl_xor(T0, 32, 64);
      value = T0 + cb[kW];
    }
  }
#pragma unroll
  for (int l = kLMax - 1; l >= 1; --l) {
    if (l < L) {
      float zb[kNS];
#pragma unroll
      for (int k = 0; k < kNS; ++k) zb[k] = (1.f - ckh[l][k] * ckh[l][k]) * hb[k];
      float w[12];
      load_units<12>(img, t.bwd[l], lane, w);
      f32x4 B[2] = {};
#pragma unroll
      for (int kk = 0; kk < kNS; ++kk)
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) B[mb] = mfma(w[kk * 2 + mb], zb[kk], B[mb]);
      compact_hidden(B, hb);
    }
  }
  f32x4 gacc = {};
  {
    float zb[kNS];
#pragma unroll
    for (int k = 0; k < kNS; ++k) zb[k] = (1.f - ckh[0][k] * ckh[0][k]) * hb[k];
    float w[8];
    load_units<8>(img, t.bwd[0], lane, w);  // unit kk (one M block: rows = input dims)
#pragma unroll
    for (int kk = 0; kk < kNS; ++kk) gacc = mfma(w[kk], zb[kk], gacc);
  }
  return gacc;
}

// -------------------------------------------------------------------------------------------------
// pair force: gpart[it][ch][D] = sum over chunk ch of the references of grad Phi(x_i - r_j)
// -------------------------------------------------------------------------------------------------
// n_sets sets of n items x against their set's m references r (rows of pitch ldx / ldr, sets x_set / r_set floats
// apart); item it = t * n + i. The chunk grid is fixed by the reference index: an item's numbers depend on its own
// row and on its reference set in its order only, not on n, on the items that share the call or on the launch.
struct PairForce {
  const float *x, *r;
  int64_t ldx, ldr, x_set, r_set, n_sets, n, m;
  float* gpart;  // [n_sets * n][pair_chunks(m)][D]
  TileNet net;
};
__host__ __device__ inline int pair_chunks(int64_t m) { return (int)((m + kChunk - 1) / kChunk); }
// the partials on the stream (the image is in place); the launcher owns the grid, the LDS size and its limit
int pair_force_partials(const PairForce& f, hipStream_t st);
// out[it][k] = inv_m sum_ch gpart[it][ch][k] (reduce_chunks), one thread per coordinate
int pair_force_reduce(const float* gpart, int64_t n_items, int n_ch, int D, double inv_m, float* out, hipStream_t st);

// coordinate k of item `it`: inv_m sum_ch gpart[it][ch][k], chunks in order, fp64
__device__ __forceinline__ float reduce_chunks(const float* __restrict__ gpart, int64_t it, int n_ch, int D, int k,
                                               double inv_m) {
  double s = 0.0;
  for (int c = 0; c < n_ch; ++c) s += (double)gpart[(it * n_ch + c) * D + k];
  return (float)(s * inv_m);
}

// -------------------------------------------------------------------------------------------------
// host side of a tile kernel
// -------------------------------------------------------------------------------------------------
inline bool tile_shape_ok(int dim, int n_layers, int width, int out_features) {
  return dim >= 1 && n_layers >= 1 && width >= 1 && out_features >= 1;
}
inline bool tile_envelope(int dim, int n_layers, int width, int out_features) {
  return tile_shape_ok(dim, n_layers, width, out_features) && dim <= 8 && width <= kW && n_layers <= kLMax;
}
inline bool tile_shape_ok(const pdeinv_mlp_shape* s) {
  return tile_shape_ok(s->dim, s->n_layers, s->width, s->out_features);
}
inline bool tile_envelope(const pdeinv_mlp_shape* s) {
  return tile_envelope(s->dim, s->n_layers, s->width, s->out_features);
}

int device_cus();  // compute units of the current device (256 if the query fails)

// Dynamic LDS above the default limit, up to the CU's 160 KiB: set at every launch (a "done once" flag per
// kernel type would be shared by kernels of one signature).
constexpr size_t kLdsMax = 160 * 1024;
template <typename K>
inline void allow_lds(K kernel) {
  (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsMax);
}

// workspaces are cut into 256-byte pieces: the offset of the next piece of `bytes`, `end` moved past it
inline size_t take(size_t& end, size_t bytes) {
  const size_t at = end;
  end += (bytes + 255) & ~(size_t)255;
  return at;
}
// workspace of a tile kernel: [image | h0y0 (W + O doubles)]; a caller may append to `total`
struct TileWs {
  ImagePlan ip;
  size_t off_img, off_h0, total;
};
inline TileWs tile_ws(const pdeinv_mlp_shape* s) {
  TileWs w{};
  w.ip = image_plan(s->dim, s->n_layers, s->width, s->out_features);
  w.off_img = take(w.total, sizeof(float) * (size_t)w.ip.ia.img_floats);
  w.off_h0 = take(w.total, sizeof(double) * (size_t)(s->width + s->out_features));
  return w;
}

}  // namespace mlpq
}  // namespace pdeinv
