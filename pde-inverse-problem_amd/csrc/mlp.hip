// mlp.hip — host drivers of the residuals for the non-parametric hypothesis V_hypothesis (gfx950).
//
// V(x) = sum_o y_o^2, y = h_L K_o + b_o, h_l = tanh(h_{l-1} K_l + b_l), h_0 = x   (core/model.py:32-62)
// Per sample the residual (kinetic_fokker_planck.py:33-58) needs g = grad_x V, V' = g.v and
// V'' = v^T Hess V v, and the trainer needs d loss / d theta (jax.value_and_grad, :60-61).
// Batched over samples this is a chain of dense GEMMs — [rows x W] x [W x W] — plus per-element
// Taylor / adjoint algebra:
//   F1  Taylor-mode forward, three streams (h, h', h'') through every layer        3P MACs / sample
//   R1  reverse chain of grad_x V (a_l, zeta_l)                                     1P
//   F2  forward-mode adjoint of that chain (abar_l, zetabar_l)                      1P
//   R2  reverse over the three forward streams                                      3P
//   G   weight gradients: sums of outer products over samples (4 stream pairs)      4P
// (24P FLOP per sample). The derivation is oracle/numpy_ref.py kfp_mlp_grad_analytic, checked
// against central finite differences.
//
// That chain is run on blocks of rows by a row engine (mlp_engine.h): the hand-written fp32-MFMA kernels of
// mlp_fused.hip for every AUTO / FUSED shape (FusedEngine below: shape envelope, zero padding, workspace), or
// rocBLAS GEMMs for the opt-in cross-check impl = LIBRARY (mlp_library.hip). This file holds what both share and
// what sits above them:
//   - the per-row loss kernel mlp_loss<D> and its one launch table (launch_mlp_loss)
//   - pdeinv_residual_kfp_mlp: three sample sets x chunks through the engine (config C5)
//   - pdeinv_residual_kmv_mlp: the general-Phi KMV residual, as pair rows through the engine (kmv_rows_run) or
//     through the narrow-net pair kernels of mlp_pairs.hip (kmv_pairs_orchestrate)
#include <math.h>

#include "common.h"
#include "mlp_engine.h"
#include "mlp_fused.h"

namespace pdeinv {

// per row: T1 = |g|^2, T2 = V'', T3 = V', T0 = V, true-potential terms (0T rows); seeds
// abar_0 = 2 c1 g; block partial sums of the 8 accumulator slots of pdeinv.h (PDEINV_GMM_ACC_*).
// The boundary slots report the set mean of V' (kinetic FP) or of V (bval: overdamped FP).
template <int D>
__global__ __launch_bounds__(kBlock) void mlp_loss(MlpLossArgs a, const float* __restrict__ G,
                                                   const float* __restrict__ X, int64_t ldx,
                                                   const float4* __restrict__ terms, float* __restrict__ abar0,
                                                   int64_t R, float* __restrict__ partials) {
  float acc[PDEINV_GMM_NACC] = {0, 0, 0, 0, 0, 0, 0, 0};
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < R; r += stride) {
    float g[D], x[D], T1 = 0.f;
#pragma unroll
    for (int i = 0; i < D; ++i) {
      g[i] = G[r * D + i];
      x[i] = X[r * ldx + i];
      T1 = fmaf(g[i], g[i], T1);
      abar0[r * D + i] = 2.f * a.c1 * g[i] + (a.uw ? X[r * ldx + 2 * D + i] : 0.f);
    }
    const float4 t = terms[r];
    const float T2 = t.y, T3 = t.x, T0 = t.z;
    const float wr = a.uw ? X[r * ldx + 3 * D] : 1.f;
    acc[PDEINV_GMM_ACC_LOSS] += a.c1 * T1 + a.c2 * T2 + a.c3 * T3 + a.c0 * wr * T0;
    if (a.set == 3) {  // KMV pair rows: -2 x Hessian mean and 2 x value mean (scaled by c2, c0)
      acc[PDEINV_GMM_ACC_HESSIAN] += -0.5f * a.c2 * T2;
      acc[PDEINV_GMM_ACC_FRICTION] += a.c0 * wr * T0;
    } else if (a.set == 0) {
      float gt[D];
      if (a.true_kind == PDEINV_POT_QUADRATIC) {
#pragma unroll
        for (int i = 0; i < D; ++i) {
          float s = 0.f;
#pragma unroll
          for (int j = 0; j < D; ++j) s = fmaf(a.tp[i * D + j], x[j], s);
          gt[i] = s;
        }
      } else {
        float w[16], amax = -INFINITY;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
          if (k < a.KT) {
            float d2 = 0.f;
#pragma unroll
            for (int i = 0; i < D; ++i) {
              const float u = x[i] - a.tp[k * D + i];
              d2 = fmaf(u, u, d2);
            }
            w[k] = -0.5f * d2 * a.l2st;
            amax = fmaxf(amax, w[k]);
          }
        }
        float den = 0.f, m[D];
#pragma unroll
        for (int i = 0; i < D; ++i) m[i] = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
          if (k < a.KT) {
            const float e = __builtin_amdgcn_exp2f(w[k] - amax);
            den += e;
#pragma unroll
            for (int i = 0; i < D; ++i) m[i] = fmaf(e, a.tp[k * D + i], m[i]);
          }
        }
        const float inv = 1.f / den;
#pragma unroll
        for (int i = 0; i < D; ++i) gt[i] = a.s2t * (x[i] - m[i] * inv);
      }
      float Tt = 0.f, Tgt = 0.f;
#pragma unroll
      for (int i = 0; i < D; ++i) {
        Tt = fmaf(gt[i], gt[i], Tt);
        Tgt = fmaf(gt[i] - g[i], gt[i] - g[i], Tgt);
      }
      acc[PDEINV_GMM_ACC_LOSS] += a.c_true * Tt;
      acc[PDEINV_GMM_ACC_LOSS_GT] += a.c_true * Tgt;
      acc[PDEINV_GMM_ACC_NABLA] += a.c_true * T1;
      acc[PDEINV_GMM_ACC_HESSIAN] += a.c_true * T2;
      acc[PDEINV_GMM_ACC_FRICTION] += a.c_true * T3;
      acc[PDEINV_GMM_ACC_NABLA_TRUE] += a.c_true * Tt;
    } else if (a.set == 1) {
      acc[PDEINV_GMM_ACC_INITIAL] += a.inv_n * (a.bval ? T0 : T3);
    } else {
      acc[PDEINV_GMM_ACC_TERMINAL] += a.inv_n * (a.bval ? T0 : T3);
    }
  }
  __shared__ float lds[kWavesPerBlock * PDEINV_GMM_NACC];
  block_reduce_to_slab(acc, PDEINV_GMM_NACC, lds, partials, blockIdx.x, gridDim.x);
}

__global__ void slab_reduce_accum_kernel(const float* __restrict__ partials, int n_blocks,
                                         double* __restrict__ out) {
  const int c = blockIdx.x;
  const float* col = partials + (int64_t)c * n_blocks;
  double s = 0.0;
  for (int b = threadIdx.x; b < n_blocks; b += kBlock) s += (double)col[b];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  __shared__ double w[kWavesPerBlock];
  if ((threadIdx.x & 63) == 0) w[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[c] += w[0] + w[1] + w[2] + w[3];
}

__global__ void kfp_terms_finalize_kernel(const double* __restrict__ acc, const float* __restrict__ grad,
                                          int64_t n_grad, float gamma, float* __restrict__ out) {
  double s = 0.0;
  for (int64_t k = threadIdx.x; k < n_grad; k += kBlock) s += (double)grad[k] * (double)grad[k];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  __shared__ double w[kWavesPerBlock];
  if ((threadIdx.x & 63) == 0) w[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    out[PDEINV_KFP_LOSS] = (float)acc[PDEINV_GMM_ACC_LOSS];
    out[PDEINV_KFP_LOSS_GT] = (float)acc[PDEINV_GMM_ACC_LOSS_GT];
    out[PDEINV_KFP_GRAD_NORM] = (float)sqrt(w[0] + w[1] + w[2] + w[3]);
    out[PDEINV_KFP_NABLA] = (float)acc[PDEINV_GMM_ACC_NABLA];
    out[PDEINV_KFP_HESSIAN] = (float)acc[PDEINV_GMM_ACC_HESSIAN];
    out[PDEINV_KFP_FRICTION] = (float)(gamma * acc[PDEINV_GMM_ACC_FRICTION]);
    out[PDEINV_KFP_NABLA_TRUE] = (float)acc[PDEINV_GMM_ACC_NABLA_TRUE];
    out[PDEINV_KFP_INITIAL] = (float)acc[PDEINV_GMM_ACC_INITIAL];
    out[PDEINV_KFP_TERMINAL] = (float)acc[PDEINV_GMM_ACC_TERMINAL];
  }
}

// The one launch table of mlp_loss: the fused engine's dims (2, 4, 8, 16) and the library engine's (1-8, 10, 12, 16).
int launch_mlp_loss(const MlpLossArgs& la, const float* G, const float* X, int64_t ldx, const float4* terms,
                    float* abar0, int64_t R, float* part, double* acc, hipStream_t st) {
  const int lg = grid_for(R) < kLossGrid ? grid_for(R) : kLossGrid;
  switch (la.d) {
#define CASE(DD) case DD: hipLaunchKernelGGL(mlp_loss<DD>, dim3(lg), dim3(kBlock), 0, st, la, G, X, ldx, terms, abar0, R, part); break;
    CASE(1) CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8) CASE(10) CASE(12) CASE(16)
#undef CASE
    default:
      return fail(PDEINV_ERR_UNSUPPORTED, "mlp: dim must be one of 1-8, 10, 12, 16");
  }
  hipLaunchKernelGGL(slab_reduce_accum_kernel, dim3(PDEINV_GMM_NACC), dim3(kBlock), 0, st, part, lg, acc);
  return PDEINV_OK;
}

}  // namespace pdeinv

using namespace pdeinv;

// ---- the fused row engine ----------------------------------------------------------------------
// The shapes the fused fp32-MFMA path takes. The kernels are compiled for dim in {2, 4, 8, 16} and width in
// {32, 64, 128, 256, 512, 1024} (any depth 1..16, any out_features: mlpf::supported); every other dim <= 16 and
// width <= 1024 runs zero-padded to the next compiled one — exact: padded inputs and K1 rows are zero, padded
// hidden units have zero weights in and out (common.h MlpPadMap) — at the cost of the padded MACs. The
// reference's default V_hypothesis is 20 wide (configurations/neural_network/MLP.yaml:4-5). Only the explicit
// impl = LIBRARY reaches the rocBLAS path; an AUTO / FUSED shape outside the envelope is UNSUPPORTED.
struct FusedShape {
  int Dp = 0, Wp = 0;
  bool pad = false;
};
static int pad_dim(int D) { return D <= 2 ? 2 : (D <= 4 ? 4 : (D <= 8 ? 8 : 16)); }
static bool fused_shape(const pdeinv_kfp_mlp_desc* d, FusedShape* f = nullptr) {
  if (d->impl == PDEINV_MLP_IMPL_LIBRARY || d->dim < 1 || d->dim > 16 || d->n_layers < 1 ||
      d->n_layers > kMlpPadMaxL || d->out_features < 1)
    return false;
  int Wp = 0;
  for (int w : {32, 64, 128, 256, 512, 1024})
    if (w >= d->width) { Wp = w; break; }
  const int Dp = pad_dim(d->dim);
  if (!Wp || !mlpf::supported(Dp, d->n_layers, Wp, d->out_features)) return false;
  if (f) { f->Dp = Dp; f->Wp = Wp; f->pad = Dp != d->dim || Wp != d->width; }
  return true;
}

// The shape runs the hand-written fused fp32-MFMA path under impl = AUTO: the padded envelope of fused_shape (dims
// and widths zero-padded to the compiled ones), not only the compiled shapes themselves.
extern "C" int pdeinv_mlp_fused_supported(int32_t dim, int32_t n_layers, int32_t width, int32_t out_features) {
  pdeinv_kfp_mlp_desc d{};
  d.dim = dim; d.n_layers = n_layers; d.width = width; d.out_features = out_features;
  d.impl = PDEINV_MLP_IMPL_AUTO;
  return fused_shape(&d) ? 1 : 0;
}

__global__ void mlp_pad_params_kernel(MlpPadMap pm, const float* __restrict__ src, int64_t P, float* __restrict__ dst) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= P) return;
  const int64_t r = pm.real_of(q);
  dst[q] = r >= 0 ? src[r] : 0.f;
}

__global__ void mlp_unpad_grad_kernel(MlpPadMap pm, const float* __restrict__ gp, int64_t P, float* __restrict__ grad) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= P) return;
  const int64_t r = pm.real_of(q);
  if (r >= 0) grad[r] += gp[q];
}

// rows [x | v] of d floats -> [x, 0.. | v, 0..] of Dp (the fused path's dim padding)
__global__ void mlp_pad_rows_kernel(const float* __restrict__ src, int64_t ld, int64_t R, int D, int Dp,
                                    float* __restrict__ dst) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= R * 2 * Dp) return;
  const int64_t r = q / (2 * Dp);
  const int c = (int)(q - r * 2 * Dp), half = c / Dp, k = c - half * Dp;
  dst[q] = k < D ? src[r * ld + half * D + k] : 0.f;
}

namespace {
struct LossCtx {
  const MlpLossArgs* la;
  const float* zr;
  int64_t ld;
  float* part;
  double* acc;
};

int fused_loss_hook(void* p, const float* G, const float4* terms, float* abar0, int64_t R, hipStream_t st) {
  const LossCtx* c = (const LossCtx*)p;
  const int rc = launch_mlp_loss(*c->la, G, c->zr, c->ld, terms, abar0, R, c->part, c->acc, st);
  return rc ? rc : check_launch("kfp_mlp fused loss");
}

struct FusedEngine final : RowEngine {
  const int D, L, O, Dp, Wp;
  const int64_t Bc;
  const bool pad;  // some dim or width is zero-padded: the chain runs on a padded parameter copy
  const std::string who;
  MlpPadMap pm{};
  int64_t PP = 0;  // padded parameter count (0: no padding)
  // workspace (floats): [run_chunk workspace | loss partials | padded params | padded gradient | padded rows]
  size_t off_part, off_pbuf, off_gbuf, off_rows, total;
  bool pad_rows;  // the caller's rows are [x | v] of D floats: copied to Dp per chunk
  float* w = nullptr;
  double* acc = nullptr;
  float* grad_out = nullptr;
  hipStream_t st = nullptr;
  int64_t poff[18], boff[18];
  mlpf::Chunk c{};

  // rows_padded: the caller builds its rows with row_dim() coordinates per block (the KMV pair rows)
  FusedEngine(const pdeinv_kfp_mlp_desc& m, const FusedShape& f, bool rows_padded, const char* who_)
      : D(m.dim), L(m.n_layers), O(m.out_features), Dp(f.Dp), Wp(f.Wp), Bc(chunk_rows_of(&m)), pad(f.pad),
        who(who_), pad_rows(!rows_padded && f.Dp != m.dim) {
    if (pad) {
      pm = mlp_pad_map(D, m.width, L, O, Dp, Wp, O);
      PP = pm.padded_count();
    }
    size_t o = 0;
    auto take = [&](size_t n) { const size_t at = o; o += (n + 63) & ~(size_t)63; return at; };
    take(mlpf::workspace_floats(Dp, L, Wp, O, Bc));
    off_part = take((size_t)PDEINV_GMM_NACC * kLossGrid);
    off_pbuf = take((size_t)PP);
    off_gbuf = take((size_t)PP);
    off_rows = take(pad_rows ? (size_t)Bc * 2 * Dp : 0);
    total = o;
  }
  int row_dim() const override { return Dp; }
  size_t ws_floats() const override { return total; }
  const float* grad_rows() const override { return mlpf::grad_rows(c); }

  int begin(const float* params, float* grad, float* ws, double* acc_, hipStream_t st_) override {
    w = ws; acc = acc_; grad_out = grad; st = st_;
    param_offsets(Dp, Wp, O, L, poff, boff);
    c = mlpf::Chunk{};
    c.d = Dp; c.L = L; c.W = Wp; c.O = O;
    c.params = params; c.grad = grad; c.poff = poff; c.boff = boff;
    c.ws = w; c.Bc = Bc;
    if (pad) {  // zero-padded copy of the parameters and a padded gradient accumulator behind the workspace
      float* pbuf = w + off_pbuf;
      float* gbuf = w + off_gbuf;
      hipLaunchKernelGGL(mlp_pad_params_kernel, dim3((unsigned)((PP + 255) / 256)), dim3(256), 0, st, pm, params, PP,
                         pbuf);
      if (hipMemsetAsync(gbuf, 0, sizeof(float) * PP, st) != hipSuccess) return fail(PDEINV_ERR_HIP, who + ": memset");
      c.params = pbuf;
      c.grad = gbuf;
    }
    return PDEINV_OK;
  }

  int chunk(const float* rows, int64_t ld, int64_t R, const MlpLossArgs& la, RowMode mode,
            const float* wrow) override {
    c.R = R;
    c.z = rows;
    c.ldz = ld;
    if (pad_rows) {
      float* prow = w + off_rows;
      const int64_t nq = R * 2 * Dp;
      hipLaunchKernelGGL(mlp_pad_rows_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, rows, ld, R, D, Dp,
                         prow);
      c.z = prow;
      c.ldz = 2 * Dp;
    }
    c.c2 = la.c2; c.c3 = la.c3; c.c0 = la.c0;
    c.wrow = wrow;
    c.ldw = wrow ? ld : 0;
    c.grad_only = mode == RowMode::GRAD_ONLY;
    c.first_order = mode == RowMode::FIRST_ORDER;
    LossCtx lc{&la, c.z, c.ldz, w + off_part, acc};
    return mlpf::run_chunk(c, mlpf::LossHook{fused_loss_hook, &lc}, st);
  }

  int end() override {
    if (!pad) return PDEINV_OK;
    hipLaunchKernelGGL(mlp_unpad_grad_kernel, dim3((unsigned)((PP + 255) / 256)), dim3(256), 0, st, pm, c.grad, PP,
                       grad_out);
    return check_launch("mlp_unpad_grad_kernel");
  }
};

// The true potential of the 0T loss terms on rows of Dp > la.d coordinates: zero rows / columns of tilde_F, zero
// coordinates of mu_k.
int pad_true_potential(MlpLossArgs& la, int Dp) {
  const int D = la.d;
  if (Dp == D) return PDEINV_OK;
  PDEINV_REQUIRE(la.true_kind == PDEINV_POT_QUADRATIC || la.KT * Dp <= PDEINV_MAX_PARAMS, PDEINV_ERR_UNSUPPORTED,
                 "kfp_mlp: padded true GMM exceeds PDEINV_MAX_PARAMS");
  const int rows = la.true_kind == PDEINV_POT_QUADRATIC ? D : la.KT;
  float tp[PDEINV_MAX_PARAMS];
  for (int k = 0; k < PDEINV_MAX_PARAMS; ++k) { tp[k] = la.tp[k]; la.tp[k] = 0.f; }
  for (int k = 0; k < rows; ++k)
    for (int i = 0; i < D; ++i) la.tp[k * Dp + i] = tp[k * D + i];
  la.d = Dp;
  return PDEINV_OK;
}

// the engine of a KFP descriptor: fused inside the envelope, else the library plan (only impl = LIBRARY runs it)
std::unique_ptr<RowEngine> kfp_engine(const pdeinv_kfp_mlp_desc* d) {
  FusedShape f;
  if (fused_shape(d, &f)) return std::make_unique<FusedEngine>(*d, f, false, "kfp_mlp");
  return make_library_engine(*d, "kfp_mlp");
}
}  // namespace

extern "C" size_t pdeinv_residual_kfp_mlp_workspace_bytes(const pdeinv_kfp_mlp_desc* d) {
  if (!d || d->dim < 1 || d->n_layers < 1 || d->width < 1 || d->out_features < 1) return 0;
  return kfp_engine(d)->ws_floats() * sizeof(float);
}

extern "C" int64_t pdeinv_mlp_param_count(int32_t dim, int32_t n_layers, int32_t width, int32_t out_features) {
  int64_t n = (int64_t)dim * width + width;
  for (int l = 1; l < n_layers; ++l) n += (int64_t)width * width + width;
  return n + (int64_t)width * out_features + out_features;
}

// ---- pdeinv_mlp_potential outside the tile envelope (sde_mlp.hip) ---------------------------------------
// Rows [x | 0] of row_dim() coordinates through the fused engine in RowMode::GRAD_ONLY, chunk by chunk: grad V is
// grad_rows(), V is terms[r].z — run_chunk_l1 and run_chunk_full both write the terms plane (E_OUT, sum_terms)
// before their grad_only return.
__global__ void mlp_pot_rows_kernel(const float* __restrict__ x, int64_t ld, int64_t R, int D, int Dp,
                                    float* __restrict__ dst) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= R * 2 * Dp) return;
  const int64_t r = q / (2 * Dp);
  const int c = (int)(q - r * 2 * Dp);
  dst[q] = c < D ? x[r * ld + c] : 0.f;
}
__global__ void mlp_pot_out_kernel(const float* __restrict__ G, const float4* __restrict__ terms, int64_t R, int D,
                                   int Dp, float* __restrict__ value, float* __restrict__ grad) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= R * D) return;
  const int64_t r = q / D;
  const int k = (int)(q - r * D);
  if (grad) grad[q] = G[r * Dp + k];
  if (value && k == 0) value[r] = terms[r].z;
}

namespace {
constexpr int64_t kPotChunk = 1 << 16;
pdeinv_kfp_mlp_desc pot_desc(const pdeinv_mlp_shape* s, int64_t n) {
  pdeinv_kfp_mlp_desc m{};
  m.dim = s->dim; m.n_layers = s->n_layers; m.width = s->width; m.out_features = s->out_features;
  m.impl = PDEINV_MLP_IMPL_AUTO;
  m.chunk_rows = n < 1 ? 1 : (n < kPotChunk ? n : kPotChunk);
  return m;
}
}  // namespace

size_t pdeinv::mlp_rows_potential_workspace_bytes(const pdeinv_mlp_shape* s, int64_t n) {
  const pdeinv_kfp_mlp_desc m = pot_desc(s, n);
  FusedShape f;
  if (!fused_shape(&m, &f)) return 0;
  const FusedEngine eng(m, f, true, "mlp_potential");
  return sizeof(float) * (eng.ws_floats() + (((size_t)m.chunk_rows * 2 * f.Dp + 63) & ~(size_t)63));
}

int pdeinv::mlp_rows_potential(const pdeinv_mlp_shape* s, const float* params, const float* x, int64_t n, int64_t ld,
                               float* value, float* grad, void* ws, hipStream_t st) {
  const pdeinv_kfp_mlp_desc m = pot_desc(s, n);
  FusedShape f;
  PDEINV_REQUIRE(fused_shape(&m, &f), PDEINV_ERR_UNSUPPORTED, "mlp_potential: shape outside the fused row envelope");
  FusedEngine eng(m, f, true, "mlp_potential");
  float* w = (float*)ws;
  float* rows = w + eng.ws_floats();
  int rc = eng.begin(params, nullptr, w, nullptr, st);
  if (rc) return rc;
  const int D = s->dim, Dp = f.Dp;
  MlpLossArgs la{};
  la.d = Dp;
  for (int64_t r0 = 0; r0 < n; r0 += m.chunk_rows) {
    const int64_t R = n - r0 < m.chunk_rows ? n - r0 : m.chunk_rows;
    const int64_t nq = R * 2 * Dp;
    hipLaunchKernelGGL(mlp_pot_rows_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, x + r0 * ld, ld, R, D,
                       Dp, rows);
    rc = eng.chunk(rows, 2 * Dp, R, la, RowMode::GRAD_ONLY, nullptr);
    if (rc) return rc;
    hipLaunchKernelGGL(mlp_pot_out_kernel, dim3((unsigned)((R * D + 255) / 256)), dim3(256), 0, st, eng.grad_rows(),
                       mlpf::term_rows(eng.c), R, D, Dp, value ? value + r0 : nullptr, grad ? grad + r0 * D : nullptr);
    rc = check_launch("mlp_pot_out_kernel");
    if (rc) return rc;
  }
  return PDEINV_OK;  // no end(): a gradient-only run has no parameter gradient to unpad
}

// ---- KFP residual (config C5) --------------------------------------------------------------------
extern "C" int pdeinv_residual_kfp_mlp(const pdeinv_kfp_mlp_desc* d, const float* zi, int64_t ni, int64_t ldi,
                                       const float* zt, int64_t nt, int64_t ldt, const float* z0, int64_t n0,
                                       int64_t ld0, const float* params, void* ws, double* acc, float* grad,
                                       void* stream) {
  PDEINV_REQUIRE(d != nullptr, PDEINV_ERR_INVALID, "kfp_mlp: null descriptor");
  const int D = d->dim;
  PDEINV_REQUIRE(D >= 1 && D <= 16, PDEINV_ERR_UNSUPPORTED, "kfp_mlp: dim must be in [1, 16]");
  PDEINV_REQUIRE(d->n_layers >= 1 && d->width >= 1 && d->out_features >= 1, PDEINV_ERR_INVALID,
                 "kfp_mlp: need n_layers, width, out_features >= 1");
  PDEINV_REQUIRE(d->impl >= PDEINV_MLP_IMPL_AUTO && d->impl <= PDEINV_MLP_IMPL_FUSED, PDEINV_ERR_INVALID,
                 "kfp_mlp: impl must be AUTO, LIBRARY or FUSED");
  PDEINV_REQUIRE(d->true_kind == PDEINV_POT_QUADRATIC || d->true_kind == PDEINV_POT_GMM, PDEINV_ERR_UNSUPPORTED,
                 "kfp_mlp: true potential must be QUADRATIC or GMM");
  PDEINV_REQUIRE(d->true_params != nullptr, PDEINV_ERR_INVALID, "kfp_mlp: true_params is null");
  PDEINV_REQUIRE(d->true_kind != PDEINV_POT_GMM || (d->n_centers_true >= 1 && d->n_centers_true <= 16 &&
                                                   d->n_centers_true * D <= PDEINV_MAX_PARAMS && d->sigma_true > 0.f),
                 PDEINV_ERR_UNSUPPORTED, "kfp_mlp: true GMM needs 1..16 centres");
  PDEINV_REQUIRE(n0 >= 1 && ni >= 0 && nt >= 0, PDEINV_ERR_INVALID, "kfp_mlp: 0T set must be non-empty");
  PDEINV_REQUIRE(params && ws && acc && grad && z0 && (ni == 0 || zi) && (nt == 0 || zt), PDEINV_ERR_INVALID,
                 "kfp_mlp: null pointer");
  // rocBLAS serves the explicit impl = LIBRARY only: AUTO / FUSED outside the hand-written envelope are rejected
  PDEINV_REQUIRE(d->impl == PDEINV_MLP_IMPL_LIBRARY || fused_shape(d), PDEINV_ERR_UNSUPPORTED,
                 "kfp_mlp: the hand-written path takes dim <= 16, 1 <= n_layers <= 16, width <= 1024 (zero-padded to "
                 "the compiled dims / widths), any out_features; impl = LIBRARY (rocBLAS) is the opt-in cross-check");
  const int64_t Bc = chunk_rows_of(d);
  PDEINV_REQUIRE(Bc <= (1 << 26), PDEINV_ERR_INVALID, "kfp_mlp: chunk_rows too large");
  hipStream_t st = (hipStream_t)stream;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return fail(PDEINV_ERR_HIP, "kfp_mlp: hipGetDevice failed");
  PDEINV_REQUIRE(d->n_layers <= 16, PDEINV_ERR_UNSUPPORTED, "kfp_mlp: at most 16 hidden layers");

  MlpLossArgs la{};
  la.d = D;
  la.true_kind = d->true_kind;
  la.KT = d->n_centers_true;
  la.s2t = d->sigma_true > 0.f ? 1.f / (d->sigma_true * d->sigma_true) : 1.f;
  la.l2st = la.s2t * 1.4426950408889634f;
  const int ntp = d->true_kind == PDEINV_POT_QUADRATIC ? D * D : d->n_centers_true * D;
  for (int k = 0; k < ntp; ++k) la.tp[k] = d->true_params[k];
  la.c_true = d->c_true;

  // boundary sets weight V' (kinetic FP, :49-50) or V itself (overdamped FP, fokker_planck.py:48-52)
  const bool bval = d->boundary_value != 0;
  la.bval = bval ? 1 : 0;
  struct Set { const float* z; int64_t n, ld; int id; float c1, c2, c3, c0; } sets[3] = {
      {z0, n0, ld0 ? ld0 : 2 * D, 0, d->c_nabla, d->c_hess, d->c_fric, 0.f},
      {zi, ni, ldi ? ldi : 2 * D, 1, 0.f, 0.f, bval ? 0.f : d->c_init, bval ? d->c_init : 0.f},
      {zt, nt, ldt ? ldt : 2 * D, 2, 0.f, 0.f, bval ? 0.f : d->c_term, bval ? d->c_term : 0.f}};

  const std::unique_ptr<RowEngine> eng = kfp_engine(d);
  int rc = eng->begin(params, grad, (float*)ws, acc, st);
  if (rc) return rc;
  rc = pad_true_potential(la, eng->row_dim());
  if (rc) return rc;
  for (const Set& s : sets) {
    PDEINV_REQUIRE(s.n == 0 || s.ld >= 2 * D, PDEINV_ERR_INVALID, "kfp_mlp: row stride < 2*dim");
    la.set = s.id; la.c1 = s.c1; la.c2 = s.c2; la.c3 = s.c3; la.c0 = s.c0;
    la.inv_n = s.n ? 1.f / (float)s.n : 0.f;
    // the initial / terminal sets weight V' (or V) only: no R1 / F2 (kinetic_fokker_planck.py:34-39)
    const RowMode mode = s.id != 0 && s.c1 == 0.f && s.c2 == 0.f ? RowMode::FIRST_ORDER : RowMode::FULL;
    for (int64_t r0 = 0; r0 < s.n; r0 += Bc) {
      const int64_t R = (s.n - r0) < Bc ? (s.n - r0) : Bc;
      rc = eng->chunk(s.z + r0 * s.ld, s.ld, R, la, mode, nullptr);
      if (rc) return rc;
    }
  }
  return eng->end();
}

// ---- KMV residual for a general (MLP) interaction Phi_theta = V_hypothesis ----------------------
// (methods/consistency_instances/kinetic_mckean_vlasov.py:11-120 under get_model non-parametric.)
// Per time stamp t the reference forms every pair (i, j) of its particles, y = x_i - x_j
// (x_minus_ref, :20-23), and needs  gbar_i = mean_j grad Phi(y_ij),  mean_j v_i^T Hess Phi(y_ij) v_i
// and  mean_j Phi(y_ij)  weighted by c_it = ds2 + ds^2 + gamma ds of log rho. The loss is quadratic
// in gbar, so its parameter adjoint is per pair once gbar is known — two passes over pair rows
// [y_ij | v_i | u_i | w_it] (built chunk by chunk, never the whole n^2 tensor):
//   pass 1  grad_x V of the pair rows (the engine's GRAD_ONLY mode), mean over j -> gbar (fp32 ws);
//           |gbar|^2, |gbar*|^2, |gbar* - gbar|^2 with gbar* = tilde_F (x_i - xbar_t) (Phi* quadratic);
//   pass 2  the full chain with c2 = -2 s, c0 = 2 s w_it and the input-gradient seed
//           u_i = 2 s gbar_i, s = 1 / (n^2 n_time)  (oracle/numpy_ref.py kmv_mlp_grad_analytic).
// rows of DP >= D floats per block: the particles' D coordinates, zeros past them (the fused path's dim padding)
template <int D, int DP = D>
__global__ void kmv_pair_rows_kernel(const float* __restrict__ z, int64_t set_stride, int64_t ld, int64_t t,
                                     int64_t i0, int64_t ni, int64_t j0, int64_t nj, int64_t n_rows,
                                     const float* __restrict__ gbar, const float* __restrict__ ds, float gamma,
                                     float u_scale, float* __restrict__ rows) {
  const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (r >= ni * nj) return;
  const int64_t il = r / nj, i = i0 + il, j = j0 + (r - il * nj);
  const float* zi = z + t * set_stride + i * ld;
  const float* zj = z + t * set_stride + j * ld;
  float* o = rows + r * (3 * DP + 1);
  const int64_t p = t * n_rows + i;
#pragma unroll
  for (int k = 0; k < DP; ++k) {
    o[k] = k < D ? zi[k] - zj[k] : 0.f;
    o[DP + k] = k < D ? zi[D + k] : 0.f;
    o[2 * DP + k] = (k < D && gbar) ? u_scale * gbar[p * D + k] : 0.f;
  }
  float wv = 0.f;
  if (ds) {
    const float a = ds[2 * p], b2 = ds[2 * p + 1];
    wv = b2 + a * a + gamma * a;  // ds2 + ds^2 + gamma ds (kinetic_mckean_vlasov.py:84-89)
  }
  o[3 * DP] = wv;
}

// gbar[t][i0 + il] += inv_n * sum_jl G[il * nj + jl] (one block per il; fixed-order LDS tree)
template <int D, int DP = D>
__global__ __launch_bounds__(kBlock) void kmv_group_mean_kernel(const float* __restrict__ G, int64_t nj, float inv_n,
                                                                float* __restrict__ gbar_rows) {
  const int64_t il = blockIdx.x;
  float s[D];
#pragma unroll
  for (int k = 0; k < D; ++k) s[k] = 0.f;
  for (int64_t jl = threadIdx.x; jl < nj; jl += kBlock) {
#pragma unroll
    for (int k = 0; k < D; ++k) s[k] += G[(il * nj + jl) * DP + k];  // G rows of DP (padded dims dropped)
  }
  __shared__ float red[kBlock];
  for (int k = 0; k < D; ++k) {
    red[threadIdx.x] = s[k];
    __syncthreads();
    for (int h = kBlock / 2; h > 0; h >>= 1) {
      if (threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
      __syncthreads();
    }
    if (threadIdx.x == 0) gbar_rows[il * D + k] += inv_n * red[0];
    __syncthreads();
  }
}

struct KmvTrueArgs {
  float F[PDEINV_MAX_DIM * PDEINV_MAX_DIM];
};

// per time stamp t (one block): xbar_t, then sum_i |gbar|^2, |gbar*|^2, |gbar* - gbar|^2 -> part[t][3]
template <int D>
__global__ __launch_bounds__(kBlock) void kmv_stamp_terms_kernel(KmvTrueArgs a, const float* __restrict__ z,
                                                                int64_t set_stride, int64_t ld, int64_t n_rows,
                                                                const float* __restrict__ gbar,
                                                                double* __restrict__ part) {
  const int64_t t = blockIdx.x;
  const float* zt = z + t * set_stride;
  __shared__ double red[kBlock];
  __shared__ float xbar[D];
  for (int k = 0; k < D; ++k) {
    double sk = 0.0;
    for (int64_t i = threadIdx.x; i < n_rows; i += kBlock) sk += (double)zt[i * ld + k];
    red[threadIdx.x] = sk;
    __syncthreads();
    for (int h = kBlock / 2; h > 0; h >>= 1) {
      if (threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
      __syncthreads();
    }
    if (threadIdx.x == 0) xbar[k] = (float)(red[0] / (double)n_rows);
    __syncthreads();
  }
  double acc[3] = {0.0, 0.0, 0.0};
  for (int64_t i = threadIdx.x; i < n_rows; i += kBlock) {
    float y[D];
#pragma unroll
    for (int k = 0; k < D; ++k) y[k] = zt[i * ld + k] - xbar[k];
    const float* g = gbar + (t * n_rows + i) * D;
    float n1 = 0.f, n2 = 0.f, n3 = 0.f;
#pragma unroll
    for (int r = 0; r < D; ++r) {
      float gt = 0.f;
#pragma unroll
      for (int c = 0; c < D; ++c) gt = fmaf(a.F[r * D + c], y[c], gt);
      n1 = fmaf(g[r], g[r], n1);
      n2 = fmaf(gt, gt, n2);
      n3 = fmaf(gt - g[r], gt - g[r], n3);
    }
    acc[0] += n1; acc[1] += n2; acc[2] += n3;
  }
  for (int c = 0; c < 3; ++c) {
    red[threadIdx.x] = acc[c];
    __syncthreads();
    for (int h = kBlock / 2; h > 0; h >>= 1) {
      if (threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
      __syncthreads();
    }
    if (threadIdx.x == 0) part[t * 3 + c] = red[0];
    __syncthreads();
  }
}

// fixed-order combine of the per-stamp sums into the PDEINV_GMM_ACC_* slots (+=)
__global__ void kmv_stamp_combine_kernel(const double* __restrict__ part, int64_t n_sets, double inv,
                                         double* __restrict__ acc) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double n1 = 0.0, n2 = 0.0, n3 = 0.0;
  for (int64_t t = 0; t < n_sets; ++t) {
    n1 += part[t * 3];
    n2 += part[t * 3 + 1];
    n3 += part[t * 3 + 2];
  }
  acc[PDEINV_GMM_ACC_LOSS] += (n1 + n2) * inv;
  acc[PDEINV_GMM_ACC_LOSS_GT] += n3 * inv;
  acc[PDEINV_GMM_ACC_NABLA] += n1 * inv;
  acc[PDEINV_GMM_ACC_NABLA_TRUE] += n2 * inv;
}

// the gbar terms of the loss, once gbar of every particle is known (after pass 1 of either route)
template <int D>
static void kmv_stamp_terms(const pdeinv_kmv_mlp_desc* d, const float* z, int64_t set_stride, int64_t ld,
                            const float* gbar, double* part, double* acc, hipStream_t st) {
  KmvTrueArgs ta{};
  for (int q = 0; q < D * D; ++q) ta.F[q] = d->tilde_F[q];
  const int64_t n = d->n_rows, T = d->n_sets;
  hipLaunchKernelGGL(kmv_stamp_terms_kernel<D>, dim3((unsigned)T), dim3(kBlock), 0, st, ta, z, set_stride, ld, n, gbar,
                     part);
  hipLaunchKernelGGL(kmv_stamp_combine_kernel, dim3(1), dim3(64), 0, st, part, T, 1.0 / ((double)n * (double)T), acc);
}

// the narrow-net pair kernels (mlp_pairs.hip): pairs generated in registers, MFMA weight gradients
namespace pdeinv {
bool kmv_pairs_supported(const pdeinv_kmv_mlp_desc* d);
bool kmvq_supported(const pdeinv_kmv_mlp_desc* d);
size_t kmv_pairs_workspace_bytes(const pdeinv_kmv_mlp_desc* d);
int kmv_pairs_run(const pdeinv_kmv_mlp_desc* d, const float* z, int64_t set_stride, int64_t ld, const float* ds,
                  const float* params, void* ws, double* acc, float* grad, float** gbar_out, int pass, hipStream_t st);
}  // namespace pdeinv

static bool kmv_use_pairs(const pdeinv_kmv_mlp_desc* d) {
  return d->impl != PDEINV_MLP_IMPL_LIBRARY && kmv_pairs_supported(d);
}

// ---- the row route: pair rows through a row engine ---------------------------------------------------
// Wide general-Phi nets (width >= 32) run their pair rows through the fused engine (the C5 machinery: B-resident
// row GEMMs, LDS-free weight gradients; widths between the compiled ones zero-padded, no rocBLAS); impl = LIBRARY
// runs the same rows through the rocBLAS engine (dim <= 8).
static pdeinv_kfp_mlp_desc kmv_as_kfp(const pdeinv_kmv_mlp_desc* d) {
  pdeinv_kfp_mlp_desc m{};
  m.dim = d->dim; m.n_layers = d->n_layers; m.width = d->width; m.out_features = d->out_features;
  m.chunk_rows = d->chunk_rows;
  m.impl = d->impl;
  return m;
}

static bool kmv_use_fused(const pdeinv_kmv_mlp_desc* d) {
  if (d->impl == PDEINV_MLP_IMPL_LIBRARY || kmv_use_pairs(d)) return false;
  if (d->dim < 1 || d->dim > 16) return false;
  const pdeinv_kfp_mlp_desc m = kmv_as_kfp(d);
  return fused_shape(&m);
}

namespace {
std::unique_ptr<RowEngine> kmv_rows_engine(const pdeinv_kmv_mlp_desc* d) {
  const pdeinv_kfp_mlp_desc m = kmv_as_kfp(d);
  FusedShape f;
  if (kmv_use_fused(d) && fused_shape(&m, &f)) return std::make_unique<FusedEngine>(m, f, true, "kmv_mlp");
  return make_library_engine(m, "kmv_mlp");
}

// the pair-row blocking and the driver's tail of the workspace, behind the engine's floats
struct KmvRowsPlan {
  int64_t ni, nj;                              // pair-row block: ni particles x nj references
  size_t off_rows, off_gbar, off_part, total;  // floats (part: doubles); total in bytes
};

KmvRowsPlan kmv_rows_plan(const pdeinv_kmv_mlp_desc* d, const RowEngine& eng) {
  const pdeinv_kfp_mlp_desc m = kmv_as_kfp(d);
  const int64_t Bc = chunk_rows_of(&m), n = d->n_rows;
  KmvRowsPlan k{};
  k.nj = n <= Bc ? n : Bc;
  k.ni = n <= Bc ? (Bc / n < n ? Bc / n : n) : 1;
  size_t o = eng.ws_floats();
  auto take = [&](size_t floats) { const size_t at = o; o += (floats + 63) & ~(size_t)63; return at; };
  k.off_rows = take((size_t)Bc * (3 * eng.row_dim() + 1));
  k.off_gbar = take((size_t)d->n_sets * n * d->dim);
  k.off_part = take((size_t)d->n_sets * 3 * 2);
  k.total = o * sizeof(float);
  return k;
}
}  // namespace

// D = the particles' dim, DP = the engine's row_dim() (fused: D zero-padded to 2 / 4 / 8 / 16, the pair rows
// carry the padding)
template <int D, int DP>
static int kmv_rows_run(const pdeinv_kmv_mlp_desc* d, RowEngine& eng, const float* z, int64_t set_stride, int64_t ld,
                        const float* ds, const float* params, float* w, double* acc, float* grad, hipStream_t st) {
  const KmvRowsPlan k = kmv_rows_plan(d, eng);
  int rc = eng.begin(params, grad, w, acc, st);
  if (rc) return rc;
  const int64_t n = d->n_rows, T = d->n_sets, rld = 3 * DP + 1;
  float* rows = w + k.off_rows;
  float* gbar = w + k.off_gbar;
  double* part = (double*)(w + k.off_part);
  const double s = 1.0 / ((double)n * (double)n * (double)T);
  if (hipMemsetAsync(gbar, 0, sizeof(float) * (size_t)T * n * D, st) != hipSuccess)
    return fail(PDEINV_ERR_HIP, "kmv_mlp: memset");
  MlpLossArgs la{};
  la.d = DP;
  for (int pass = 0; pass < 2; ++pass) {
    if (pass == 1) {
      la.set = 3; la.uw = 1;
      la.c1 = 0.f; la.c3 = 0.f; la.c2 = (float)(-2.0 * s); la.c0 = (float)(2.0 * s);
    }
    for (int64_t t = 0; t < T; ++t) {
      for (int64_t i0 = 0; i0 < n; i0 += k.ni) {
        const int64_t ni = (n - i0) < k.ni ? (n - i0) : k.ni;
        for (int64_t j0 = 0; j0 < n; j0 += k.nj) {
          const int64_t nj = (n - j0) < k.nj ? (n - j0) : k.nj;
          const int64_t R = ni * nj;
          hipLaunchKernelGGL((kmv_pair_rows_kernel<D, DP>), dim3(grid_for(R)), dim3(kBlock), 0, st, z, set_stride, ld,
                             t, i0, ni, j0, nj, n, pass ? gbar : nullptr, pass ? ds : nullptr, d->gamma,
                             (float)(2.0 * s), rows);
          rc = eng.chunk(rows, rld, R, la, pass ? RowMode::FULL : RowMode::GRAD_ONLY, pass ? rows + 3 * DP : nullptr);
          if (rc) return rc;
          if (pass == 0)
            hipLaunchKernelGGL((kmv_group_mean_kernel<D, DP>), dim3((unsigned)ni), dim3(kBlock), 0, st,
                               eng.grad_rows(), nj, (float)(1.0 / (double)n), gbar + (t * n + i0) * D);
        }
      }
    }
    if (pass == 0) kmv_stamp_terms<D>(d, z, set_stride, ld, gbar, part, acc, st);
  }
  rc = eng.end();
  return rc ? rc : check_launch("kmv_mlp kernels");
}

static size_t kmv_pairs_part_offset(const pdeinv_kmv_mlp_desc* d) { return (kmv_pairs_workspace_bytes(d) + 255) & ~(size_t)255; }

extern "C" int pdeinv_kmv_mlp_path(const pdeinv_kmv_mlp_desc* d) {
  if (!d || d->dim < 1 || d->n_layers < 1 || d->n_layers > 16 || d->width < 1 || d->out_features < 1) return -1;
  if (kmv_use_pairs(d)) return kmvq_supported(d) ? PDEINV_KMV_PATH_PAIR_TILES : PDEINV_KMV_PATH_PAIR_RING;
  if (d->impl == PDEINV_MLP_IMPL_PAIRS_RING) return -1;
  if (kmv_use_fused(d)) return PDEINV_KMV_PATH_FUSED_ROWS;
  // rocBLAS only on the explicit opt-in, and only for the shapes its kernels take (dim 1..8)
  return d->impl == PDEINV_MLP_IMPL_LIBRARY && d->dim <= 8 ? PDEINV_KMV_PATH_LIBRARY : -1;
}

extern "C" size_t pdeinv_residual_kmv_mlp_workspace_bytes(const pdeinv_kmv_mlp_desc* d) {
  if (!d || d->dim < 1 || d->n_layers < 1 || d->width < 1 || d->out_features < 1 || d->n_sets < 1 || d->n_rows < 1)
    return 0;
  if (kmv_use_pairs(d)) return kmv_pairs_part_offset(d) + sizeof(double) * (size_t)d->n_sets * 3;
  return kmv_rows_plan(d, *kmv_rows_engine(d)).total;
}

template <int D>
static int kmv_pairs_orchestrate(const pdeinv_kmv_mlp_desc* d, const float* z, int64_t set_stride, int64_t ld,
                                 const float* ds, const float* params, void* ws, double* acc, float* grad,
                                 hipStream_t st) {
  float* gbar = nullptr;
  int rc = kmv_pairs_run(d, z, set_stride, ld, ds, params, ws, acc, grad, &gbar, 0, st);
  if (rc) return rc;
  double* part = (double*)((char*)ws + kmv_pairs_part_offset(d));
  kmv_stamp_terms<D>(d, z, set_stride, ld, gbar, part, acc, st);
  rc = check_launch("kmv_stamp kernels");
  if (rc) return rc;
  return kmv_pairs_run(d, z, set_stride, ld, ds, params, ws, acc, grad, nullptr, 1, st);
}

extern "C" int pdeinv_residual_kmv_mlp(const pdeinv_kmv_mlp_desc* d, const float* z, int64_t set_stride, int64_t ld,
                                       const float* ds, const float* params, void* ws, double* acc, float* grad,
                                       void* stream) {
  PDEINV_REQUIRE(d != nullptr, PDEINV_ERR_INVALID, "kmv_mlp: null descriptor");
  PDEINV_REQUIRE(d->n_layers >= 1 && d->n_layers <= 16 && d->width >= 1 && d->out_features >= 1, PDEINV_ERR_INVALID,
                 "kmv_mlp: need 1 <= n_layers <= 16, width, out_features >= 1");
  PDEINV_REQUIRE(d->n_sets >= 1 && d->n_rows >= 1, PDEINV_ERR_INVALID, "kmv_mlp: need n_sets, n_rows >= 1");
  PDEINV_REQUIRE(ld >= 2 * d->dim && set_stride >= 0, PDEINV_ERR_INVALID, "kmv_mlp: row stride < 2*dim");
  PDEINV_REQUIRE(z && ds && params && ws && acc && grad && d->tilde_F, PDEINV_ERR_INVALID, "kmv_mlp: null pointer");
  PDEINV_REQUIRE(d->impl >= PDEINV_MLP_IMPL_AUTO && d->impl <= PDEINV_MLP_IMPL_PAIRS_RING, PDEINV_ERR_INVALID,
                 "kmv_mlp: impl must be AUTO, LIBRARY, FUSED or PAIRS_RING");
  PDEINV_REQUIRE(d->impl != PDEINV_MLP_IMPL_PAIRS_RING || kmv_use_pairs(d), PDEINV_ERR_UNSUPPORTED,
                 "kmv_mlp: PAIRS_RING needs dim <= 8, width <= 28, n_layers <= 16, out_features <= 64");
  PDEINV_REQUIRE(pdeinv_kmv_mlp_path(d) >= 0, PDEINV_ERR_UNSUPPORTED,
                 "kmv_mlp: the hand-written paths need dim <= 8 with width <= 28 (pair kernels), or dim <= 16 with "
                 "1 <= n_layers <= 16, width <= 1024 (fused MFMA path); impl = LIBRARY (rocBLAS, dim <= 8) is the "
                 "opt-in cross-check");
  hipStream_t st = (hipStream_t)stream;
  if (kmv_use_pairs(d)) {
    switch (d->dim) {
#define CASE(DD) case DD: return kmv_pairs_orchestrate<DD>(d, z, set_stride, ld, ds, params, ws, acc, grad, st);
      CASE(1) CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8)
#undef CASE
    }
  }
  // the library engine computes in the particles' dim (1..8), the fused engine in the next compiled one
  const std::unique_ptr<RowEngine> eng = kmv_rows_engine(d);
  switch (d->dim * 32 + eng->row_dim()) {
#define CASE(DD, DDP) \
  case DD * 32 + DDP: return kmv_rows_run<DD, DDP>(d, *eng, z, set_stride, ld, ds, params, (float*)ws, acc, grad, st);
    CASE(1, 1) CASE(2, 2) CASE(3, 3) CASE(4, 4) CASE(5, 5) CASE(6, 6) CASE(7, 7) CASE(8, 8)
    CASE(1, 2) CASE(3, 4) CASE(5, 8) CASE(6, 8) CASE(7, 8)
    CASE(9, 16) CASE(10, 16) CASE(11, 16) CASE(12, 16) CASE(13, 16) CASE(14, 16) CASE(15, 16) CASE(16, 16)
#undef CASE
    default:
      return fail(PDEINV_ERR_UNSUPPORTED, "kmv_mlp: dim must be in [1, 8]");
  }
}

extern "C" int pdeinv_kfp_terms_finalize(const double* acc, const float* grad, int64_t n_grad, float gamma,
                                         float* out, void* stream) {
  PDEINV_REQUIRE(acc && grad && out && n_grad >= 0, PDEINV_ERR_INVALID, "kfp_terms_finalize: bad arguments");
  hipLaunchKernelGGL(kfp_terms_finalize_kernel, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, acc, grad, n_grad,
                     gamma, out);
  return check_launch("kfp_terms_finalize_kernel");
}
