// mlp_library.hip — the rocBLAS row engine of the V_hypothesis residuals (impl = LIBRARY), gfx950.
//
// The opt-in cross-check of the hand-written kernels (mlp_fused.hip): the residual chain of mlp.hip (F1 / R1 /
// loss / F2 / R2 / G) with every GEMM a plain library GEMM (rocBLAS sgemm, fp32 on the MFMA f32 path) and every
// element-wise step a kernel below. No AUTO / FUSED shape reaches this file; the per-row loss terms are mlp.hip's
// mlp_loss (launch_mlp_loss), shared with the fused engine. Interface: mlp_engine.h.
#include <dlfcn.h>

#include <atomic>
#include <math.h>
#include <rocblas/rocblas.h>

#include "common.h"
#include "mlp_engine.h"

namespace pdeinv {

// ---- rocBLAS plumbing ------------------------------------------------------------------------
// rocBLAS serves only the explicit opt-in impl = LIBRARY (a cross-check of the hand-written kernels): every AUTO /
// FUSED shape runs on this library's own kernels. So libpdeinv.so does not link it: the first LIBRARY call loads
// librocblas.so.5 with dlopen and resolves the five entry points it uses; without it that call fails loudly
// (PDEINV_ERR_UNSUPPORTED), and no other path notices. (rocblas.h supplies the types only.)
struct BlasApi {
  decltype(&rocblas_create_handle) create_handle = nullptr;
  decltype(&rocblas_destroy_handle) destroy_handle = nullptr;
  decltype(&rocblas_set_stream) set_stream = nullptr;
  decltype(&rocblas_sgemm) sgemm = nullptr;
  decltype(&rocblas_sgemm_strided_batched) sgemm_strided_batched = nullptr;
  bool ok = false;
};

// residual calls served by rocBLAS in this process (pdeinv_rocblas_calls: AUTO / FUSED never add to it)
static std::atomic<int64_t> g_rocblas_calls{0};

static const BlasApi& blas_api() {
  static const BlasApi api = [] {
    BlasApi a{};
    void* lib = nullptr;
    for (const char* name : {"librocblas.so.5", "/opt/rocm/lib/librocblas.so.5", "librocblas.so"}) {
      lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
      if (lib) break;
    }
    if (!lib) return a;
    a.create_handle = (decltype(a.create_handle))dlsym(lib, "rocblas_create_handle");
    a.destroy_handle = (decltype(a.destroy_handle))dlsym(lib, "rocblas_destroy_handle");
    a.set_stream = (decltype(a.set_stream))dlsym(lib, "rocblas_set_stream");
    a.sgemm = (decltype(a.sgemm))dlsym(lib, "rocblas_sgemm");
    a.sgemm_strided_batched = (decltype(a.sgemm_strided_batched))dlsym(lib, "rocblas_sgemm_strided_batched");
    a.ok = a.create_handle && a.destroy_handle && a.set_stream && a.sgemm && a.sgemm_strided_batched;
    return a;
  }();
  return api;
}

// One handle per (host thread, device): a rocBLAS handle carries its stream, so a handle shared
// between threads lets one thread's rocblas_set_stream retarget another thread's GEMMs (the ABI
// promises reentrancy across distinct streams, include/pdeinv.h). Thread-local handles need no lock
// around set_stream + the GEMM sequence; they are destroyed when the thread exits.
struct ThreadBlasHandles {
  rocblas_handle h[64] = {};
  ~ThreadBlasHandles() {
    for (rocblas_handle& x : h)
      if (x) blas_api().destroy_handle(x);
  }
};

static rocblas_handle blas_handle(int device) {
  thread_local ThreadBlasHandles handles;
  if (device < 0 || device >= 64 || !blas_api().ok) return nullptr;
  if (!handles.h[device]) {
    if (blas_api().create_handle(&handles.h[device]) != rocblas_status_success) handles.h[device] = nullptr;
  }
  return handles.h[device];
}

// K-split factor of the weight-gradient GEMMs: the reduction runs over 4 x chunk rows while the
// output is only n_in x n_out (<= 256 x 256), so one GEMM launches a few dozen workgroups. Slicing
// the rows into up to kMaxKSplit batched GEMMs (>= kMinKSlice rows each) fills the chip; the fp32
// partial slabs are summed in a fixed order (deterministic, no atomics).
constexpr int kMaxKSplit = 256;
constexpr int64_t kMinKSlice = 4096;
constexpr int kColsumBlocks = 512;

// out[i] += sum_k part[k * n + i]. A block owns kSumCols outputs; its kBlock / kSumCols thread
// groups each sum a strided subset of the S slices (independent loads in flight), then the group
// partials are added in a fixed order through LDS — deterministic, and fast for the small n
// (a few thousand weights) and large S of the weight / bias gradients.
constexpr int kSumCols = 32;
__global__ __launch_bounds__(kBlock) void sum_slices_kernel(const float* __restrict__ part, int S, int64_t n,
                                                            float* __restrict__ out) {
  constexpr int G = kBlock / kSumCols;
  __shared__ float red[G][kSumCols];
  const int c = threadIdx.x % kSumCols, g = threadIdx.x / kSumCols;
  const int64_t i = (int64_t)blockIdx.x * kSumCols + c;
  float s = 0.f;
  if (i < n)
    for (int k = g; k < S; k += G) s += part[(int64_t)k * n + i];
  red[g][c] = s;
  __syncthreads();
  if (g == 0 && i < n) {
    float t = 0.f;
#pragma unroll
    for (int q = 0; q < G; ++q) t += red[q][c];
    out[i] += t;
  }
}

// partial column sums of B[R x n] (row-major): block b sums rows [b*rpb, (b+1)*rpb). For n < kBlock
// the block's threads cover kBlock / n rows at a time (lane t: column t % n, row offset t / n), so
// every thread is busy and a wave reads contiguous bytes; the row-lanes are combined in a fixed
// order through LDS. Wider outputs use blockIdx.y column tiles of kBlock.
__global__ __launch_bounds__(kBlock) void colsum_partial_kernel(const float* __restrict__ B, int64_t R, int n,
                                                                int64_t rpb, float* __restrict__ part) {
  __shared__ float red[kBlock];
  const int64_t r0 = (int64_t)blockIdx.x * rpb;
  const int64_t r1 = r0 + rpb < R ? r0 + rpb : R;
  if (n >= kBlock) {
    const int c = blockIdx.y * kBlock + threadIdx.x;
    if (c >= n) return;
    float s = 0.f;
    for (int64_t r = r0; r < r1; ++r) s += B[r * n + c];
    part[(int64_t)blockIdx.x * n + c] = s;
    return;
  }
  const int lanes = kBlock / n;  // row-lanes (>= 1)
  const int c = threadIdx.x % n, q = threadIdx.x / n;
  float s = 0.f;
  if (q < lanes)
    for (int64_t r = r0 + q; r < r1; r += lanes) s += B[r * n + c];
  red[threadIdx.x] = s;
  __syncthreads();
  if (q == 0) {
    float t = 0.f;
    for (int k = 0; k < lanes; ++k) t += red[k * n + c];
    part[(int64_t)blockIdx.x * n + c] = t;
  }
}

struct Blas {
  rocblas_handle h;
  hipStream_t st;
  float* part;  // >= kMaxKSplit * max(n_in * n_out) floats (also holds the colsum partials)
  int status = 0;
  // row-major C[R x n_out] = A[R x n_in] . K[n_in x n_out]
  void fwd(const float* A, const float* K, float* C, int64_t R, int n_in, int n_out) {
    const float one = 1.f, zero = 0.f;
    if (blas_api().sgemm(h, rocblas_operation_none, rocblas_operation_none, n_out, (rocblas_int)R, n_in, &one, K,
                      n_out, A, n_in, &zero, C, n_out) != rocblas_status_success)
      status = 1;
  }
  // row-major C[R x n_in] = A[R x n_out] . K^T
  void bwd(const float* A, const float* K, float* C, int64_t R, int n_in, int n_out) {
    const float one = 1.f, zero = 0.f;
    if (blas_api().sgemm(h, rocblas_operation_transpose, rocblas_operation_none, n_in, (rocblas_int)R, n_out, &one, K,
                      n_out, A, n_out, &zero, C, n_in) != rocblas_status_success)
      status = 1;
  }
  // Kbar[n_in x n_out] += A[R x n_in]^T . B[R x n_out]  (K-split into S batched slices + slab sum)
  void wgrad(const float* A, const float* B, float* Kbar, int64_t R, int n_in, int n_out) {
    const float one = 1.f, zero = 0.f;
    int64_t S = R / kMinKSlice;
    S = S < 1 ? 1 : (S > kMaxKSplit ? kMaxKSplit : S);
    const int64_t Ks = R / S, rem = R - S * Ks;
    const int64_t nout = (int64_t)n_in * n_out;
    if (blas_api().sgemm_strided_batched(h, rocblas_operation_none, rocblas_operation_transpose, n_out, n_in,
                                      (rocblas_int)Ks, &one, B, n_out, Ks * n_out, A, n_in, Ks * n_in, &zero, part,
                                      n_out, nout, (rocblas_int)S) != rocblas_status_success)
      status = 1;
    hipLaunchKernelGGL(sum_slices_kernel, dim3(grid_for(nout, kSumCols)), dim3(kBlock), 0, st, part, (int)S, nout, Kbar);
    if (rem > 0 && blas_api().sgemm(h, rocblas_operation_none, rocblas_operation_transpose, n_out, n_in,
                                 (rocblas_int)rem, &one, B + S * Ks * n_out, n_out, A + S * Ks * n_in, n_in, &one,
                                 Kbar, n_out) != rocblas_status_success)
      status = 1;
  }
  // bbar[n] += sum over the R rows of B[R x n]
  void colsum(const float* B, float* bbar, int64_t R, int n) {
    const int64_t rpb = (R + kColsumBlocks - 1) / kColsumBlocks;
    const int nb = (int)((R + rpb - 1) / rpb);
    hipLaunchKernelGGL(colsum_partial_kernel, dim3(nb, n >= kBlock ? (n + kBlock - 1) / kBlock : 1), dim3(kBlock), 0,
                       st, B, R, n, rpb, part);
    hipLaunchKernelGGL(sum_slices_kernel, dim3(grid_for(n, kSumCols)), dim3(kBlock), 0, st, part, nb, (int64_t)n, bbar);
  }
};

// ---- element-wise kernels --------------------------------------------------------------------
__device__ __forceinline__ float fast_tanh(float z) {
  // tanh(z) = 1 - 2 / (exp(2z) + 1); exp2 on the hardware unit, saturates cleanly at +-1
  const float e = __builtin_amdgcn_exp2f(2.8853900817779268f * z);
  return 1.f - 2.f * __builtin_amdgcn_rcpf(e + 1.f);
}

// F1: z (+bias), z', z'' -> h = tanh z, h' = s1 z', h'' = s1 z'' + s2 z'^2
__global__ void mlp_act_fwd(const float* __restrict__ Z, float* __restrict__ A, const float* __restrict__ bias,
                            int64_t R, int n) {
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t S = R * n;
  if (e >= S) return;
  const int j = (int)(e % n);
  const float z = Z[e] + bias[j], zd = Z[S + e], zdd = Z[2 * S + e];
  const float h = fast_tanh(z);
  const float s1 = 1.f - h * h, s2 = -2.f * h * s1;
  A[e] = h;
  A[S + e] = s1 * zd;
  A[2 * S + e] = fmaf(s1, zdd, s2 * zd * zd);
}

// output layer: y (+bias) stored back; u = 2y (seed of the grad_x chain); per row
// terms = {V' = 2 y.y', V'' = 2(y'.y' + y.y''), V = y.y, 0}
// A block owns rb consecutive rows = rb*O consecutive elements of each plane: phase 1 is
// element-wise and coalesced, the per-element products go to LDS, phase 2 sums them per row.
__global__ __launch_bounds__(kBlock) void mlp_out(float* __restrict__ Y, const float* __restrict__ bias,
                                                  float* __restrict__ YB, float4* __restrict__ terms, int64_t R,
                                                  int O, int rb) {
  extern __shared__ float prod[];  // [3][rb*O]
  const int64_t S = R * O;
  const int64_t r0 = (int64_t)blockIdx.x * rb;
  const int nr = (int)((R - r0) < rb ? (R - r0) : rb);
  const int ne = nr * O;
  const int64_t e0 = r0 * O;
  for (int k = threadIdx.x; k < ne; k += kBlock) {
    const int64_t e = e0 + k;
    const float y = Y[e] + bias[k % O], yd = Y[S + e], ydd = Y[2 * S + e];
    Y[e] = y;
    YB[3 * S + e] = 2.f * y;
    prod[k] = y * yd;
    prod[rb * O + k] = fmaf(yd, yd, y * ydd);
    prod[2 * rb * O + k] = y * y;
  }
  __syncthreads();
  for (int r = threadIdx.x; r < nr; r += kBlock) {
    float vd = 0.f, vdd = 0.f, v = 0.f;
    for (int o = 0; o < O; ++o) {
      vd += prod[r * O + o];
      vdd += prod[rb * O + r * O + o];
      v += prod[2 * rb * O + r * O + o];
    }
    terms[r0 + r] = make_float4(2.f * vd, 2.f * vdd, v, 0.f);
  }
}

// R1: zeta = tanh'(z) * a   (a = GEMM output, kept for R2)
__global__ void mlp_gchain(const float* __restrict__ a, const float* __restrict__ h, float* __restrict__ zeta,
                           int64_t S) {
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (e >= S) return;
  const float hv = h[e];
  zeta[e] = (1.f - hv * hv) * a[e];
}

// F2: abar = tanh'(z) * zetabar
__global__ void mlp_gadj(const float* __restrict__ zetabar, const float* __restrict__ h, float* __restrict__ abar,
                         int64_t S) {
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (e >= S) return;
  const float hv = h[e];
  abar[e] = (1.f - hv * hv) * zetabar[e];
}

// seeds of the reverse sweep over the forward streams (c0: weight of the value V = y.y):
//   ybar = 2 c3 y' + 2 c2 y'' + 2 ubar + 2 c0 y,  y'bar = 2 c3 y + 4 c2 y',  y''bar = 2 c2 y
// (rw: optional per-row weight of the value term, rw[r * ldw] for element e = r * O + o)
__global__ void mlp_seeds(const float* __restrict__ Y, const float* __restrict__ UB, float* __restrict__ YB,
                          float c2, float c3, float c0, int64_t S, const float* __restrict__ rw, int64_t ldw, int O) {
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (e >= S) return;
  const float y = Y[e], yd = Y[S + e], ydd = Y[2 * S + e];
  const float cv = rw ? c0 * rw[(e / O) * ldw] : c0;
  YB[e] = 2.f * c3 * yd + 2.f * c2 * ydd + 2.f * UB[e] + 2.f * cv * y;
  YB[S + e] = 2.f * c3 * y + 4.f * c2 * yd;
  YB[2 * S + e] = 2.f * c2 * y;
}

// R2 element-wise step through tanh (s1 = tanh', s2 = tanh'', s3 = tanh'''):
//   zbar   = s1 hbar + s2 z' h'bar + (s2 z'' + s3 z'^2) h''bar + s2 a zetabar   (last: grad_x chain)
//   z'bar  = s1 h'bar + 2 s2 z' h''bar ;   z''bar = s1 h''bar
__global__ void mlp_act_bwd(const float* __restrict__ HB, const float* __restrict__ h, const float* __restrict__ Z,
                            const float* __restrict__ aL, const float* __restrict__ zb, float* __restrict__ ZB,
                            int64_t S) {
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (e >= S) return;
  const float hv = h[e];
  const float s1 = 1.f - hv * hv, s2 = -2.f * hv * s1, s3 = -2.f * s1 * s1 - 2.f * hv * s2;
  const float zd = Z[S + e], zdd = Z[2 * S + e];
  const float hb = HB[e], hdb = HB[S + e], hddb = HB[2 * S + e];
  ZB[e] = s1 * hb + s2 * zd * hdb + (s2 * zdd + s3 * zd * zd) * hddb + s2 * aL[e] * zb[e];
  ZB[S + e] = s1 * hdb + 2.f * s2 * zd * hddb;
  ZB[2 * S + e] = s1 * hddb;
}

// copy the (x, v) rows of a sample set into the stream-0 / stream-1 input planes of layer 1
__global__ void mlp_load_rows(const float* __restrict__ z, int64_t ld, int d, float* __restrict__ A0, int64_t R) {
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (e >= R * d) return;
  const int64_t r = e / d;
  const int i = (int)(e - r * d);
  A0[e] = z[r * ld + i];
  A0[R * d + e] = z[r * ld + d + i];
}

// ---- workspace plan -------------------------------------------------------------------------
struct MlpPlan {
  int d, L, W, O;
  int64_t Bc;
  size_t off_A0, off_Y, off_YB, off_UB, off_G, off_kpart, off_terms, off_part, total;
  size_t off_layer0, layer_stride;  // per hidden layer: A(4) Z(3) ZB(4) HB(3) aL(1) zb(1) planes of Bc*W
};

static MlpPlan make_plan(const pdeinv_kfp_mlp_desc* d) {
  MlpPlan p{};
  p.d = d->dim; p.L = d->n_layers; p.W = d->width; p.O = d->out_features;
  p.Bc = chunk_rows_of(d);
  size_t o = 0;
  auto take = [&](size_t floats) { const size_t at = o; o += (floats + 63) & ~(size_t)63; return at; };
  p.off_A0 = take(4 * p.Bc * p.d);
  p.off_Y = take(3 * p.Bc * p.O);
  p.off_YB = take(4 * p.Bc * p.O);
  p.off_UB = take(p.Bc * p.O);
  p.off_G = take(p.Bc * p.d);
  const int64_t wmax = (int64_t)p.W * (p.W > p.d ? (p.W > p.O ? p.W : p.O) : p.d);
  const int64_t cmax = (int64_t)kColsumBlocks * (p.W > p.O ? p.W : p.O);
  p.off_kpart = take((size_t)(kMaxKSplit * wmax > cmax ? kMaxKSplit * wmax : cmax));
  p.off_terms = take(4 * p.Bc);
  p.off_part = take((size_t)PDEINV_GMM_NACC * kLossGrid);
  p.layer_stride = 16 * p.Bc * p.W;
  p.off_layer0 = take(p.layer_stride * p.L);
  p.total = o * sizeof(float);
  return p;
}

// ---- the engine ------------------------------------------------------------------------------
namespace {
struct LibraryEngine final : RowEngine {
  const MlpPlan p;
  const std::string who;
  Blas blas{};
  float* w = nullptr;
  const float* params = nullptr;
  float* grad = nullptr;
  int64_t poff[18], boff[18];
  hipStream_t st = nullptr;
  double* acc = nullptr;
  int64_t R = 0;

  LibraryEngine(const pdeinv_kfp_mlp_desc& m, const char* who_) : p(make_plan(&m)), who(who_) {}
  int row_dim() const override { return p.d; }
  size_t ws_floats() const override { return p.total / sizeof(float); }
  const float* grad_rows() const override { return w + p.off_G; }
  int end() override { return PDEINV_OK; }

  int begin(const float* params_, float* grad_, float* ws, double* acc_, hipStream_t st_) override {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return fail(PDEINV_ERR_HIP, who + ": hipGetDevice failed");
    w = ws; params = params_; grad = grad_; acc = acc_; st = st_;
    blas = Blas{blas_handle(dev), st, w + p.off_kpart};
    PDEINV_REQUIRE(blas_api().ok, PDEINV_ERR_UNSUPPORTED,
                   who + ": impl = LIBRARY needs rocBLAS (librocblas.so.5 could not be loaded)");
    if (!blas.h) return fail(PDEINV_ERR_HIP, who + ": rocblas_create_handle failed");
    if (blas_api().set_stream(blas.h, st) != rocblas_status_success)
      return fail(PDEINV_ERR_HIP, who + ": rocblas_set_stream");
    g_rocblas_calls.fetch_add(1, std::memory_order_relaxed);
    param_offsets(p.d, p.W, p.O, p.L, poff, boff);
    return PDEINV_OK;
  }

  float* layer(int l, int plane) const {
    return w + p.off_layer0 + p.layer_stride * (l - 1) + (size_t)plane * R * p.W;
  }

  // One chunk of R rows: F1 Taylor forward, R1 grad_x chain, the loss terms (mlp_loss, accumulated into
  // acc), F2 forward adjoint, R2 + weight gradients (accumulated into grad). GRAD_ONLY stops after R1 and
  // leaves g = grad_x V of every row in grad_rows(); FIRST_ORDER runs the full chain (its extra terms are zero).
  int chunk(const float* zr, int64_t ld, int64_t rows, const MlpLossArgs& la, RowMode mode,
            const float* wrow) override {
    R = rows;
    const int D = p.d, W = p.W, O = p.O, L = p.L;
    float* A0 = w + p.off_A0;
    float* Y = w + p.off_Y;
    float* YB = w + p.off_YB;
    float* UB = w + p.off_UB;
    float* Gp = w + p.off_G;
    float4* terms = (float4*)(w + p.off_terms);
    float* part = w + p.off_part;
    Blas& b = blas;
    // planes per hidden layer l: A 0-3, Z 4-6, ZB 7-10, HB 11-13, aL 14, zb 15. Inside a chunk of R
    // rows the planes are packed at stride R*W so that consecutive streams form one [k*R x W] operand.
    const int64_t SD = R * D, SW = R * W, SO = R * O;
    // ---- F1: Taylor-mode forward --------------------------------------------------------
    hipLaunchKernelGGL(mlp_load_rows, dim3(grid_for(SD)), dim3(kBlock), 0, st, zr, ld, D, A0, R);
    if (hipMemsetAsync(A0 + 2 * SD, 0, sizeof(float) * SD, st) != hipSuccess) return fail(PDEINV_ERR_HIP, "memset");
    for (int l = 1; l <= L; ++l) {
      const int n_in = (l == 1) ? D : W;
      const float* Ain = (l == 1) ? A0 : layer(l - 1, 0);
      float* Z = layer(l, 4);
      b.fwd(Ain, params + poff[l - 1], Z, 3 * R, n_in, W);  // three streams: one GEMM with 3R rows
      hipLaunchKernelGGL(mlp_act_fwd, dim3(grid_for(SW)), dim3(kBlock), 0, st, Z, layer(l, 0), params + boff[l - 1],
                         R, W);
    }
    b.fwd(layer(L, 0), params + poff[L], Y, 3 * R, W, O);
    {
      const int rb = O >= 2048 ? 1 : 2048 / O;  // 24 KB of LDS products per block
      hipLaunchKernelGGL(mlp_out, dim3((unsigned)((R + rb - 1) / rb)), dim3(kBlock), 3 * rb * O * sizeof(float), st,
                         Y, params + boff[L], YB, terms, R, O, rb);
    }
    // ---- R1: grad_x chain ---------------------------------------------------------------
    b.bwd(YB + 3 * SO, params + poff[L], layer(L, 14), R, W, O);  // a_L = u K_o^T
    for (int l = L; l >= 1; --l) {
      hipLaunchKernelGGL(mlp_gchain, dim3(grid_for(SW)), dim3(kBlock), 0, st, layer(l, 14), layer(l, 0),
                         layer(l, 10), SW);  // zeta_l -> ZB plane 3
      if (l > 1) b.bwd(layer(l, 10), params + poff[l - 1], layer(l - 1, 14), R, W, W);
      else b.bwd(layer(1, 10), params + poff[0], Gp, R, D, W);  // g = zeta_1 K_1^T
    }
    if (mode == RowMode::GRAD_ONLY) {
      if (b.status) return fail(PDEINV_ERR_HIP, "mlp: rocBLAS call failed");
      return check_launch("mlp grad_x kernels");
    }
    // ---- loss terms, seed abar_0 = 2 c1 g (+ u) ------------------------------------------
    const int rc = launch_mlp_loss(la, Gp, zr, ld, terms, A0 + 3 * SD, R, part, acc, st);
    if (rc) return rc;
    // ---- F2: forward-mode adjoint of the grad_x chain --------------------------------------
    for (int l = 1; l <= L; ++l) {
      const float* abar_prev = (l == 1) ? A0 + 3 * SD : layer(l - 1, 3);
      b.fwd(abar_prev, params + poff[l - 1], layer(l, 15), R, (l == 1) ? D : W, W);  // zetabar_l
      hipLaunchKernelGGL(mlp_gadj, dim3(grid_for(SW)), dim3(kBlock), 0, st, layer(l, 15), layer(l, 0),
                         layer(l, 3), SW);  // abar_l -> A plane 3
    }
    b.fwd(layer(L, 3), params + poff[L], UB, R, W, O);  // ubar = abar_L K_o
    hipLaunchKernelGGL(mlp_seeds, dim3(grid_for(SO)), dim3(kBlock), 0, st, Y, UB, YB, la.c2, la.c3, la.c0, SO, wrow,
                       ld, O);
    // ---- R2 + G: reverse over the three forward streams, weight gradients ---------------------
    b.wgrad(layer(L, 0), YB, grad + poff[L], 4 * R, W, O);  // K_o += [h;h';h'';abar]^T [ybar;..;u]
    b.colsum(YB, grad + boff[L], R, O);
    b.bwd(YB, params + poff[L], layer(L, 11), 3 * R, W, O);  // hbar streams of layer L
    for (int l = L; l >= 1; --l) {
      hipLaunchKernelGGL(mlp_act_bwd, dim3(grid_for(SW)), dim3(kBlock), 0, st, layer(l, 11), layer(l, 0),
                         layer(l, 4), layer(l, 14), layer(l, 15), layer(l, 7), SW);
      const int n_in = (l == 1) ? D : W;
      const float* Ain = (l == 1) ? A0 : layer(l - 1, 0);
      b.wgrad(Ain, layer(l, 7), grad + poff[l - 1], 4 * R, n_in, W);
      b.colsum(layer(l, 7), grad + boff[l - 1], R, W);
      if (l > 1) b.bwd(layer(l, 7), params + poff[l - 1], layer(l - 1, 11), 3 * R, W, W);
    }
    if (b.status) return fail(PDEINV_ERR_HIP, "mlp: rocBLAS call failed");
    return check_launch("mlp kernels");
  }
};
}  // namespace

std::unique_ptr<RowEngine> make_library_engine(const pdeinv_kfp_mlp_desc& m, const char* who) {
  return std::make_unique<LibraryEngine>(m, who);
}

}  // namespace pdeinv

extern "C" int64_t pdeinv_rocblas_calls(void) {
  return pdeinv::g_rocblas_calls.load(std::memory_order_relaxed);
}
