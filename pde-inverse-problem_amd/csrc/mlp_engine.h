// mlp_engine.h — the row engine of the V_hypothesis (MLP) residuals (internal interface).
//
// A row engine takes a block of R rows [x | v | ...] at a stride and runs the residual chain of mlp.hip on them
// (F1 / R1 / loss / F2 / R2 / G): it adds the loss slots into acc and the parameter gradient into grad. The two
// drivers of mlp.hip (pdeinv_residual_kfp_mlp, pdeinv_residual_kmv_mlp) are written once against this interface.
// It has exactly two implementations:
//   fused    the hand-written fp32-MFMA kernels of mlp_fused.hip (every AUTO / FUSED shape): mlp.hip FusedEngine
//   library  rocBLAS GEMMs + element-wise kernels (impl = LIBRARY, the opt-in cross-check): mlp_library.hip
#pragma once
#include <memory>

#include "common.h"

namespace pdeinv {

constexpr int kLossGrid = 512;
constexpr int64_t kDefaultChunkRows = 1 << 18;  // rows per chunk where the descriptor leaves chunk_rows at 0

inline int64_t chunk_rows_of(const pdeinv_kfp_mlp_desc* d) {
  return d->chunk_rows > 0 ? d->chunk_rows : kDefaultChunkRows;
}

// parameter offsets (flax order: K_1, b_1, ..., K_L, b_L, K_o, b_o)
inline void param_offsets(int D, int W, int O, int L, int64_t* poff, int64_t* boff) {
  int64_t o = 0;
  for (int l = 0; l <= L; ++l) {
    const int n_in = (l == 0) ? D : W, n_out = (l == L) ? O : W;
    poff[l] = o; o += (int64_t)n_in * n_out;
    boff[l] = o; o += n_out;
  }
}

struct MlpLossArgs {
  int d, set, true_kind, KT, bval;
  int uw;  // rows carry [x | v | u | w]: input-gradient seed u (added to abar_0) and value weight w
           // (KMV pair rows, set 3: pdeinv_residual_kmv_mlp)
  float c1, c2, c3, c0, c_true, inv_n;
  float s2t, l2st;
  float tp[PDEINV_MAX_PARAMS];  // tilde_F [d*d] or true GMM centres [K*d]
};

// The per-row loss terms of both engines (mlp.hip mlp_loss<la.d> + the fp64 slab reduce into acc): rows X at stride
// ldx, g = grad_x V in G [R x la.d], terms[r] = {V', V'', V, 0}; writes abar0 [R x la.d]. part: 8 * kLossGrid floats.
int launch_mlp_loss(const MlpLossArgs& la, const float* G, const float* X, int64_t ldx, const float4* terms,
                    float* abar0, int64_t R, float* part, double* acc, hipStream_t st);

enum class RowMode {
  FULL,
  FIRST_ORDER,  // the set weights only V' (and V): the engine may skip R1 / F2 (mlp_fused.h Chunk::first_order)
  GRAD_ONLY,    // stop after g = grad_x V of every row, left in grad_rows() (KMV pass 1)
};

struct RowEngine {
  virtual ~RowEngine() = default;
  // coordinates per x / v / u block of a row, as the engine computes them (dim, or dim zero-padded)
  virtual int row_dim() const = 0;
  // floats the engine owns at the front of the workspace (a multiple of 64); the driver's own buffers follow
  virtual size_t ws_floats() const = 0;
  // once per residual call, before the first chunk. fused: the zero-padded parameter copy and a zeroed padded
  // gradient; library: the thread's rocBLAS handle on the stream, counted in pdeinv_rocblas_calls
  virtual int begin(const float* params, float* grad, float* ws, double* acc, hipStream_t st) = 0;
  // R <= chunk rows at stride ld. wrow: per-row weight of la.c0 at the same stride (nullptr: 1)
  virtual int chunk(const float* rows, int64_t ld, int64_t R, const MlpLossArgs& la, RowMode mode,
                    const float* wrow) = 0;
  // g = grad_x V [R x row_dim()] of the last chunk
  virtual const float* grad_rows() const = 0;
  // after the last chunk. fused with padding: adds the unpadded gradient into grad
  virtual int end() = 0;
};

// pdeinv_mlp_potential outside the 16-row tile envelope (sde_mlp.hip): rows [x | 0] through the fused engine in
// RowMode::GRAD_ONLY; grad V from grad_rows(), V from the terms plane (mlp.hip). ld >= dim; either output nullable.
size_t mlp_rows_potential_workspace_bytes(const pdeinv_mlp_shape* s, int64_t n);
int mlp_rows_potential(const pdeinv_mlp_shape* s, const float* params, const float* x, int64_t n, int64_t ld,
                       float* value, float* grad, void* ws, hipStream_t st);

// who: the entry point's name in error messages ("kfp_mlp" / "kmv_mlp")
std::unique_ptr<RowEngine> make_library_engine(const pdeinv_kfp_mlp_desc& m, const char* who);

}  // namespace pdeinv
