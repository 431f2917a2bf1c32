// mlp_tile_wide.h — the 16-particle fp32-MFMA tile of a wide hypothesis net (core/model.py:32-62: tanh layers,
// Dense(out), sum of squares; dim <= 8, width 21..256 zero-padded to Wp = 16 MB, Wp * n_layers <= 512,
// out_features <= 64): the forward chain h_l = tanh(h_{l-1} K_l + b_l), y = h_L K_o + b_o and the reverse chain
// from ybar = 2 y through K_o^T, (1 - h_l^2) and K_l^T to g = grad_x V, V = sum y^2. Used by both kernels of
// sde_mlp_wide.hip. It reuses ftanh, mfma, lane_dims, allow_lds, take, device_cus and kLdsMax of mlp_tile.h and the
// waves' slot sizes of sde_mlp_tile.h.
//
// Layout. Every product is a v_mfma_f32_16x16x4_f32 with the particle on lane & 15 (the N column) and the weights
// as the A operand. The C fragment of a product's output block mo holds feature 16 mo + 4 g + r in register r of
// lane group g = lane >> 4 (the P layout of mlp_tile.h), and that register is directly the B operand of k-step r
// of input block mo of the next product: the unit permutation lives in the weight fragments. A "quad-unit" is the
// A operand of the four k-steps of one (output block, input block) pair: one f32x4 per lane, 1 KiB per wave.
//
// Activations. The checkpoints h_l ([L][MB] f32x4 per lane, up to 128 registers' worth at Wp * L = 512) are
// indexed by the run-time layer and block, so they live in a per-wave LDS region in lane-linear order: a lane
// reads back only what it wrote (no cross-lane traffic, no barrier), one ds_read_b128 per input block. The reverse
// chain overwrites them in place: slot (l, mo) turns from h_l into zbar_l = (1 - h_l^2) hbar_l when the product
// that yields hbar_l's block mo retires. y (at most four blocks) stays in registers.
//
// Weights. wide_image_kernel lays the quad-units out in the order the tile body consumes them — forward layer 0,
// forward layers 1..L-1, the output layer, its transpose, the transposes of layers L-1..1, the transpose of layer
// 0 — padded to whole slices of kQS quad-units (8 KiB), followed by the biases. An image that fits in LDS beside
// the waves' regions is staged once. A larger one cycles through two slice buffers: every wave of the block
// consumes the current slice while the block's threads hold the next slice's global loads in registers; at the
// slice boundary they write them to the other buffer and one __syncthreads() hands it over. Every wave of a block
// therefore runs the same number of tiles and updates (a wave without a tile computes on a clamped row and stores
// nothing).
#pragma once
#include "common.h"
#include "mlp_tile.h"
#include "sde_mlp_tile.h"

namespace pdeinv {
namespace mlpw {

using mlpq::allow_lds;
using mlpq::device_cus;
using mlpq::ftanh;
using mlpq::kLdsMax;
using mlpq::kSlotG;
using mlpq::kSlotZ;
using mlpq::lane_dims;
using mlpq::mfma;
using mlpq::take;

constexpr int kQS = 8;           // quad-units per slice
constexpr int kUnit = 256;       // floats per quad-unit (64 lanes x f32x4)
constexpr int kSlice4 = kQS * 64;  // f32x4 per slice
constexpr int kWavesMax = 8;     // waves per block, at most
constexpr int kWavesStream = 4;  // waves per block a streamed image needs (two slice registers per thread)
constexpr int kOBMax = 4;        // output blocks: out_features <= 64

// What the kernels need of the net and its image (kernel argument).
struct WideNet {
  int L, D, W, O, MB, OB;
  int units;        // quad-units of the image, padded to whole slices
  int n_slices;     // units / kQS
  int resident;     // the whole image is staged once
  int bias_floats;  // L * Wp + 64
  int waves;        // waves per block
  const float* img; // [units * kUnit | bias_floats]
};

__host__ __device__ inline int wide_units(int L, int MB, int OB) {
  return 2 * (MB + (L - 1) * MB * MB + OB * MB);
}

inline bool wide_shape_ok(int dim, int n_layers, int width, int out_features) {
  return dim >= 1 && n_layers >= 1 && width >= 1 && out_features >= 1;
}
inline bool wide_envelope(int dim, int n_layers, int width, int out_features) {
  if (!wide_shape_ok(dim, n_layers, width, out_features)) return false;
  if (dim > 8 || width <= mlpq::kW || width > 256 || out_features > 16 * kOBMax) return false;
  return (int64_t)16 * ((width + 15) / 16) * n_layers <= 512;
}

// LDS floats of one wave: the checkpoints and the two slots
inline size_t wide_wave_floats(int L, int MB) { return (size_t)L * MB * kUnit + kSlotG + kSlotZ; }

// The plan: image size, residency and waves per block. Resident when the image fits beside at least kWavesStream
// waves; otherwise streamed through two slice buffers. Inside the envelope streaming always fits kWavesStream
// waves: 16 KiB of slices, at most (512 + 64) * 4 B of biases and 4 x 34 KiB of wave regions (Wp * L = 512) stay
// under the CU's 160 KiB, so a streamed block has the 256 threads that the two slice registers per thread assume.
inline WideNet wide_net(int dim, int L, int width, int out_features, const float* img) {
  WideNet t{};
  t.L = L; t.D = dim; t.W = width; t.O = out_features;
  t.MB = (width + 15) / 16; t.OB = (out_features + 15) / 16;
  const int u = wide_units(L, t.MB, t.OB);
  t.units = (u + kQS - 1) / kQS * kQS;
  t.n_slices = t.units / kQS;
  t.bias_floats = L * 16 * t.MB + 16 * kOBMax;
  t.img = img;
  const size_t per_wave = sizeof(float) * wide_wave_floats(L, t.MB);
  const size_t fix_res = sizeof(float) * ((size_t)t.units * kUnit + t.bias_floats);
  const size_t fix_str = sizeof(float) * ((size_t)2 * kQS * kUnit + t.bias_floats);
  auto fit = [&](size_t fixed) {
    if (fixed + per_wave > kLdsMax) return 0;
    const size_t w = (kLdsMax - fixed) / per_wave;
    return (int)(w < (size_t)kWavesMax ? w : (size_t)kWavesMax);
  };
  const int w_res = fit(fix_res), w_str = fit(fix_str);
  t.resident = w_res >= kWavesStream;
  t.waves = t.resident ? w_res : w_str;
  return t;
}
inline size_t wide_image_floats(const WideNet& t) { return (size_t)t.units * kUnit + t.bias_floats; }
inline size_t wide_lds_bytes(const WideNet& t) {
  const size_t w = t.resident ? (size_t)t.units * kUnit : (size_t)2 * kQS * kUnit;
  return sizeof(float) * (w + t.bias_floats + (size_t)t.waves * wide_wave_floats(t.L, t.MB));
}

// -------------------------------------------------------------------------------------------------
// the image, from the flat flax vector (per layer: kernel [in][out], bias [out])
// -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void wide_image_kernel(WideNet t, const float* __restrict__ params,
                                                         float* __restrict__ img) {
  const int64_t total = (int64_t)t.units * kUnit + t.bias_floats;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int D = t.D, W = t.W, O = t.O, MB = t.MB, OB = t.OB, L = t.L, Wp = 16 * MB;
  auto roff = [&](int l) -> int64_t {  // flat offset of layer l's kernel
    return l == 0 ? 0 : (int64_t)D * W + W + (int64_t)(l - 1) * ((int64_t)W * W + W);
  };
  float v = 0.f;
  if (idx < (int64_t)t.units * kUnit) {
    int u = (int)(idx >> 8);
    const int lane = (int)(idx >> 2) & 63, r = (int)idx & 3, i = lane & 15, g = lane >> 4;
    const int kf = 4 * g + r;  // feature of k-step r within an input block
    bool done = false;
    if (u < MB) {  // forward layer 0: k-step r carries coordinate 4 r + g
      const int in = 4 * r + g, out = 16 * u + i;
      if (r < 2 && in < D && out < W) v = params[(int64_t)in * W + out];
      done = true;
    } else u -= MB;
    for (int l = 1; l < L && !done; ++l) {
      if (u < MB * MB) {
        const int in = 16 * (u % MB) + kf, out = 16 * (u / MB) + i;
        if (in < W && out < W) v = params[roff(l) + (int64_t)in * W + out];
        done = true;
      } else u -= MB * MB;
    }
    if (!done) {
      if (u < OB * MB) {  // output layer
        const int in = 16 * (u % MB) + kf, out = 16 * (u / MB) + i;
        if (in < W && out < O) v = params[roff(L) + (int64_t)in * O + out];
        done = true;
      } else u -= OB * MB;
    }
    if (!done) {
      if (u < MB * OB) {  // K_o^T: rows = hidden features, k = outputs
        const int row = 16 * (u / OB) + i, col = 16 * (u % OB) + kf;
        if (row < W && col < O) v = params[roff(L) + (int64_t)row * O + col];
        done = true;
      } else u -= MB * OB;
    }
    for (int l = L - 1; l >= 1 && !done; --l) {
      if (u < MB * MB) {  // K_l^T
        const int row = 16 * (u / MB) + i, col = 16 * (u % MB) + kf;
        if (row < W && col < W) v = params[roff(l) + (int64_t)row * W + col];
        done = true;
      } else u -= MB * MB;
    }
    if (!done && u < MB) {  // K_0^T: rows = coordinates
      const int col = 16 * u + kf;
      if (i < D && col < W) v = params[(int64_t)i * W + col];
    }
  } else {
    const int j = (int)(idx - (int64_t)t.units * kUnit);
    if (j < L * Wp) {
      const int l = j / Wp, f = j % Wp;
      if (f < W) v = params[roff(l) + (int64_t)(l == 0 ? D : W) * W + f];
    } else {
      const int f = j - L * Wp;
      if (f < O) v = params[roff(L) + (int64_t)W * O + f];
    }
  }
  img[idx] = v;
}

inline int wide_build_image(const WideNet& t, const float* params, float* img, hipStream_t st) {
  const int64_t total = (int64_t)wide_image_floats(t);
  hipLaunchKernelGGL(wide_image_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, t, params, img);
  return check_launch("wide_image_kernel");
}

// -------------------------------------------------------------------------------------------------
// the weight feed: quad-units in consumption order, resident or through two slice buffers
// -------------------------------------------------------------------------------------------------
struct Feed {
  const f32x4* gimg;  // the device image
  const f32x4* buf;   // LDS: the whole image (resident) or two slices
  int resident, n_slices;
  int nthr;  // threads of the block, from the plan (reading blockDim costs a dependent global load)
  int upos;  // resident: next unit of the image; streamed: next unit of the current slice
  int par;   // buffer of the current slice
  int nxt;   // slice held in `pre`
  f32x4 pre[2];
};

__device__ __forceinline__ void feed_prefetch(Feed& f) {
  const f32x4* src = f.gimg + (size_t)f.nxt * kSlice4;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int q = threadIdx.x + k * f.nthr;
    if (q < kSlice4) f.pre[k] = src[q];
  }
}

// Stage the biases and the image (or its first slice). All threads call; ends with a barrier.
__device__ __forceinline__ void feed_init(Feed& f, const WideNet& t, f32x4* lds4) {
  const f32x4* src = reinterpret_cast<const f32x4*>(t.img);
  const int nb4 = t.bias_floats / 4, nthr = t.waves * kWave;
  f32x4* w4 = lds4 + nb4;
  for (int q = threadIdx.x; q < nb4; q += nthr) lds4[q] = src[(size_t)t.units * 64 + q];
  const int n4 = t.resident ? t.units * 64 : kSlice4;
  for (int q = threadIdx.x; q < n4; q += nthr) w4[q] = src[q];
  f.gimg = src; f.nthr = nthr; f.buf = w4; f.resident = t.resident; f.n_slices = t.n_slices;
  f.upos = 0; f.par = 0; f.nxt = t.n_slices > 1 ? 1 : 0;
  f.pre[0] = f.pre[1] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (!t.resident) feed_prefetch(f);
  __syncthreads();
}

// The lane's f32x4 of the next quad-unit. Streamed: at a slice boundary the block writes the prefetched slice to
// the idle buffer (every wave left it before the last barrier), synchronises and starts the next prefetch.
__device__ __forceinline__ f32x4 next_unit(Feed& f, int lane) {
  if (!f.resident && f.upos == kQS) {
    f32x4* dst = const_cast<f32x4*>(f.buf) + (f.par ^ 1) * kSlice4;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int q = threadIdx.x + k * f.nthr;
      if (q < kSlice4) dst[q] = f.pre[k];
    }
    __syncthreads();
    f.par ^= 1;
    f.nxt = f.nxt + 1 == f.n_slices ? 0 : f.nxt + 1;
    feed_prefetch(f);
    f.upos = 0;
  }
  const int at = f.resident ? f.upos : f.par * kQS + f.upos;
  ++f.upos;
  return f.buf[at * 64 + lane];
}

// The image has been consumed once: the next unit is the image's first again.
__device__ __forceinline__ void feed_rewind(Feed& f) { f.upos = f.resident ? 0 : kQS; }

// sum over KB input blocks of (quad-unit) x (the lane's f32x4 of block kb at in[kb * 64]), four accumulators
// (one per k-step of a quad-unit) so that consecutive MFMAs are independent; c0 carries the bias.
__device__ __forceinline__ f32x4 dot_units(Feed& f, int lane, const f32x4* in, int KB, f32x4 c0) {
  f32x4 c1 = {0.f, 0.f, 0.f, 0.f}, c2 = c1, c3 = c1;
  f32x4 w = next_unit(f, lane), b = in[0];
  for (int kb = 0; kb < KB; ++kb) {
    f32x4 wn = w, bn = b;
    if (kb + 1 < KB) {  // the next block's operands are on their way under this block's MFMAs
      wn = next_unit(f, lane);
      bn = in[(kb + 1) * 64];
    }
    c0 = mfma(w[0], b[0], c0);
    c1 = mfma(w[1], b[1], c1);
    c2 = mfma(w[2], b[2], c2);
    c3 = mfma(w[3], b[3], c3);
    w = wn; b = bn;
  }
  return (c0 + c1) + (c2 + c3);
}

__device__ __forceinline__ f32x4 tanh4(f32x4 z) { return f32x4{ftanh(z[0]), ftanh(z[1]), ftanh(z[2]), ftanh(z[3])}; }

// V(x) and grad V(x) of the 16 particles of a tile. bias4: the LDS copy of the biases; act: the wave's checkpoint
// region ([L][MB][64] f32x4); x: coordinates 4 kk + g of the lane's particle (lane_dims<2>, zero past D). Returns
// the last product's C fragment: register r of lane (particle, g) is dV / dx_{4 g + r} (zero past D). VALUE:
// `value` = V of the lane's particle (the same on its four lane groups). Consumes the image exactly once.
template <bool VALUE>
__device__ __forceinline__ f32x4 wide_grad(const WideNet& t, Feed& f, const f32x4* bias4, f32x4* act, int lane,
                                           const float (&x)[2], float& value) {
  const int g = lane >> 4, L = t.L, MB = t.MB, OB = t.OB;
  f32x4* al = act + lane;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  for (int mo = 0; mo < MB; ++mo) {  // layer 0: the coordinates are the B operand
    const f32x4 w = next_unit(f, lane);
    f32x4 c0 = bias4[4 * mo + g], c1 = zero;
    c0 = mfma(w[0], x[0], c0);
    c1 = mfma(w[1], x[1], c1);
    al[mo * 64] = tanh4(c0 + c1);
  }
  for (int l = 1; l < L; ++l) {
    const f32x4* in = al + (l - 1) * MB * 64;
    f32x4* out = al + l * MB * 64;
    for (int mo = 0; mo < MB; ++mo) out[mo * 64] = tanh4(dot_units(f, lane, in, MB, bias4[4 * (l * MB + mo) + g]));
  }
  f32x4* top = al + (L - 1) * MB * 64;
  f32x4 y[kOBMax];
#pragma unroll
  for (int mo = 0; mo < kOBMax; ++mo) {
    y[mo] = zero;
    if (mo < OB) y[mo] = dot_units(f, lane, top, MB, bias4[4 * (L * MB + mo) + g]);
  }
  if constexpr (VALUE) {  // the particle's outputs sit on its four lane groups
    float s = 0.f;
#pragma unroll
    for (int mo = 0; mo < kOBMax; ++mo)
#pragma unroll
      for (int r = 0; r < 4; ++r) s = fmaf(y[mo][r], y[mo][r], s);
    s += __shfl_xor(s, 16, 64);
    s += __shfl_xor(s, 32, 64);
    value = s;
  }
#pragma unroll
  for (int mo = 0; mo < kOBMax; ++mo) y[mo] *= 2.f;
  for (int mo = 0; mo < MB; ++mo) {  // hbar_L = K_o ybar, then zbar_L in place
    f32x4 c[4] = {zero, zero, zero, zero};
#pragma unroll
    for (int kb = 0; kb < kOBMax; ++kb) {
      if (kb < OB) {
        const f32x4 w = next_unit(f, lane);
#pragma unroll
        for (int r = 0; r < 4; ++r) c[r] = mfma(w[r], y[kb][r], c[r]);
      }
    }
    const f32x4 h = top[mo * 64];
    top[mo * 64] = (1.f - h * h) * ((c[0] + c[1]) + (c[2] + c[3]));
  }
  for (int l = L - 1; l >= 1; --l) {
    const f32x4* in = al + l * MB * 64;
    f32x4* out = al + (l - 1) * MB * 64;
    for (int mo = 0; mo < MB; ++mo) {
      const f32x4 hb = dot_units(f, lane, in, MB, zero);
      const f32x4 h = out[mo * 64];
      out[mo * 64] = (1.f - h * h) * hb;
    }
  }
  const f32x4 ga = dot_units(f, lane, al, MB, zero);
  feed_rewind(f);
  return ga;
}

}  // namespace mlpw
}  // namespace pdeinv
