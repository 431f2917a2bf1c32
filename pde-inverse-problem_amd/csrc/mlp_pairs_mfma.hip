// mlp_pairs_mfma.hip — the general-Phi KMV residual for the reference's narrow hypothesis nets on
// the matrix pipe: 16-pair tiles, every product a v_mfma_f32_16x16x4_f32 (gfx950).
//
// Same contract as the register-ring pair kernels of mlp_pairs.hip (which stay for the shapes this
// file does not cover): for methods/consistency_instances/kinetic_mckean_vlasov.py:11-120 with a
// non-parametric Phi_theta = V_hypothesis (core/model.py:32-62: tanh layers, Dense(40), sum of
// squares), every pair (i, j) of a time stamp's particles, y_ij = x_i - x_j (x_minus_ref, :20-23),
// contributes grad Phi(y_ij) (pass 1: gbar_i = mean_j grad Phi — the pair force below, which is also the
// learned interaction of sde_mf_mlp.hip, with x = r = z per time stamp), and pass 2 differentiates
//     l_ij = u_i . grad Phi(y_ij) + c2 v_i^T Hess Phi(y_ij) v_i + c0_i Phi(y_ij)
// (u_i = 2 s gbar_i, c2 = -2 s, c0_i = 2 s w_it; s = 1 / (n^2 n_sets); loss assembly :74-97) with
// respect to theta. Covered: dim <= 8, width <= 20 (zero-padded to 20), 1 <= n_layers <= 8, any
// out_features (the output layer is folded into a 20 x 20 quadratic form) — the reference default is
// 2 -> 20 x 8 -> 40 (configurations/neural_network/MLP.yaml:4-5, model.py:45-47).
//
// Layout. A wave owns 16 pairs (i, j..j+15) of one particle i. Every activation tile is the C/D
// fragment of a 16x16x4 MFMA: the pair on lane & 15 (the MFMA's N), the feature on (lane >> 4,
// register) — "P layout". A width-20 layer output is two 16-row M blocks; its 20 real features sit in
// 5 "compact slots" (registers 0..3 of block 0, register 0 of block 1: block-1 row r = 4g + s holds
// feature 16 + 4s + g), and because an MFMA's K index is lane >> 4 within a k-step, slot k of the
// P layout is directly the B operand of k-step k of the next product: layers chain in registers, no
// LDS, no lane movement (the weights are the A operand, permuted once on the host side of the image).
//
// Pass 2 streams (Taylor mode, tanh layers): primal h, first order along u (z'_u), first and second
// order along v (z'_v, z''_v). Per tanh layer the four pre-activation streams (h, z'_u, z'_v, z''_v)
// are the whole checkpoint — 20 registers for a 16-pair tile — kept in VGPRs through the reverse sweep
// (8 layers: 145 VGPRs). Reverse: the four adjoints z-bar from the output seeds; weight gradients
// sum outer products over pairs, i.e. a contraction over the pair index, which the P layout cannot feed
// (pairs sit on the MFMA's N lanes): each stream's z-bar and layer input go through a per-wave LDS image
// [feature][pair] (pitch 24 floats: conflict-free 16-B reads, 2-way-free 4-B writes) and are read back
// with the pair on the K lanes ("F layout"); the bias gradient rides a constant-1 input row. Tile sums
// fold into the block's LDS gradient slab (ds_add_f32), copied to a per-block global slab at the end;
// a fixed-order fp64 reduction over blocks gives the gradient.
//
// Weights: one image per call (kmvq_image_kernel), lane-linear A-operand fragments of every product
// (forward: K^T with rows = outputs; backward: K with rows = inputs), staged once per persistent block
// into LDS and read as 16-B fragments.
//
// Pair force (pair_force_kernel, declared in mlp_tile.h). A wave owns one (item, chunk of kChunk references
// by reference index) unit, walks the chunk in 16-pair tiles — y = x_i - r_j formed in fp32 — and runs
// mlpq::tile_grad on each. The tile gradients of a lane add up in registers in tile order, the 16 lanes of a
// coordinate fold in a fixed butterfly, and the unit's D sums go to gpart[item][chunk]. No atomics. Tail
// tiles and the short last chunk load from a clamped row (load_ref); their pairs run the tile at y = 0 and
// are dropped by a select. The chunk partials of an item are summed in chunk order in fp64 and scaled by a
// double 1/m (reduce_chunks), by pair_force_reduce_kernel or at the head of sde_mf_mlp.hip's update.
#include <math.h>
#include <stdlib.h>

#include <type_traits>

#include "common.h"
#include "mlp_tile.h"  // kW, kNS, kLMax, the P-layout helpers, the image plan

namespace pdeinv {
namespace mlpq {

constexpr int kWaves = 8;   // waves per block of the pair force (two blocks per CU = 4 waves per SIMD)
constexpr int kWaves2 = 4;   // waves per block of pass 2: one per SIMD (512 registers: the checkpoints stay in registers)
constexpr int kPS = 28;     // LDS image row pitch (floats); odd rows shifted by one 16-byte chunk (img_at)
constexpr int kRowsA = 48, kRowsB = 32;
constexpr int kTImg = (kRowsA + kRowsB) * kPS;  // floats per wave: the [A | B] transpose images

struct Args {  // pass 2
  int n_ch;
  int64_t n, n_units, set_stride, ld;
  const float* z;
  const float* ds;
  float gamma, s;
  TileNet net;
  int qoff[kLMax + 1], qoff_out;  // gradient-slab offsets (padded layout); the output layer's
  int P;                          // padded parameter count
  const float* gbar;      // [n_items][D]
  float* gslab;           // [n_blocks][P]
  float* aslab;           // [n_waves][8]
};

// v_mfma_f32_4x4x1_16b_f32: 16 independent 4 x 4 outer products; lane 4b + j, register i of the result
// is block b's A[lane 4b + i] * B[lane 4b + j] (tools/mfma4_probe.hip; ~0.7 of the 16x16x4 issue rate)
__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_4x4x1f32(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ int pos_of(int p) { return 4 * (p & 3) + (p >> 2); }

// Transpose-image addressing: element (row, pair position pos) at row * 28 + pos, odd rows one 16-byte
// chunk further right. Pitch 28 puts the two lane groups of a put_slots ds_write_b32 (rows 4 apart) on
// opposite bank halves, and the shift keeps get_rows' ds_read_b128 lane groups on 16 distinct chunks;
// with the edge table below the edge reads are conflict-free as well (bank model: the 24-float pitch had
// 2-way conflicts on every slot write and on half of the edge reads — SQ_LDS_BANK_CONFLICT was 35 % of
// the LDS-active cycles of pass 2, profiles/r03_kmv_pairs_mfma_final_pmc.txt).
__device__ __forceinline__ int img_at(int row, int pos) { return row * kPS + pos + 4 * (row & 1); }
__device__ __forceinline__ int img_chunk(int row, int c) { return row * kPS + 4 * (c + (row & 1)); }

// Opaque copy: the reverse sweep recomputes s1, s2 and the layer-input streams from the checkpoint;
// without this the compiler CSEs them with the forward's values and keeps those live across the whole
// tile (~64 VGPRs per layer instead of the 20 of the checkpoint).
template <int N>
__device__ __forceinline__ void launder(float (&v)[N]) {
#pragma unroll
  for (int k = 0; k < N; ++k) asm volatile("" : "+v"(v[k]));
}

// P layout -> image rows (row = feature): slot k of lane (p, g) holds feature slot_feat(NS, k, g)
template <int NS>
__device__ __forceinline__ void put_slots(float* T, const float (&v)[NS], int p, int g) {
  const int pp = pos_of(p);
#pragma unroll
  for (int k = 0; k < NS; ++k) T[img_at(slot_feat(NS, k, g), pp)] = v[k];
}
// F layout read: rows 16 blk + (lane & 15), the pairs (lane >> 4) + 4 ks of k-steps ks = 0..3
__device__ __forceinline__ f32x4 get_rows(const float* T, int blk, int p, int g) {
  return *reinterpret_cast<const f32x4*>(T + img_chunk(16 * blk + p, g));
}

// Hidden-layer weight gradient dK[in][out] (+ the bias row in = 20) of one 16-pair tile: the 16 x 16
// core (in, out < 16) on 16x16x4 (every row and column real), the 164 edge entries (in 16..20 x out 0..19,
// in 0..15 x out 16..19) as 14 of the 16 blocks of one 4x4x1 MFMA per pair-stream — 4 + 16 MFMAs per
// stream instead of 16 16x16x4 over a 32 x 32 tile of which 21 x 20 is real. Block b of the edge MFMA:
// b < 8: in 16 + 4 (b >> 2) + i x out 4 (b & 3) + j;  b < 12: in 4 (b - 8) + i x out 16 + j;
// b < 14: in 16 + 4 (b - 12) + i x out 16 + j  (i: the A lane of the block, j: the B lane).
struct EdgeMap;
__device__ __forceinline__ void fold_ce(float* sl, const f32x4& G0, const f32x4& E, const EdgeMap& em, int pq, int gq,
                                        int lane, float* dump);
// Edge block of lane group b (in0 / 4, out0 / 4 as nibbles b of these words): the 14 blocks in 16..20 x
// 0..19 and 0..15 x 16..19, placed so that each ds_read_b128 lane group ({b 0,3,5,6}, {1,2,4,7},
// {8,11,13,14}, {9,10,12,15}) reads at most 8 distinct image rows, on distinct chunks (a search over the
// bank model); b = 3 and 7 are unused and read their group's first block (broadcast), never folded.
constexpr uint64_t kEdgeIn = 0x4404155345542542ull, kEdgeOut = 0x3442423401414004ull;
struct EdgeMap {
  int ra, rb;  // image rows read by this lane: hprev feature (A), zbar feature (B)
  int in0, out0;
  bool live;
  __device__ __forceinline__ explicit EdgeMap(int lane) {
    const int b = lane >> 2, i = lane & 3;
    in0 = 4 * (int)((kEdgeIn >> (4 * b)) & 15);
    out0 = 4 * (int)((kEdgeOut >> (4 * b)) & 15);
    live = b != 3 && b != 7;
    ra = in0 + i;   // <= 23: rows 21..23 of the input image are never folded
    rb = out0 + i;  // <= 19
  }
};

// Fold one tile's width-20 weight gradient into the wave's slab region sl (row-major [21][20], row 20 =
// the bias): core register r = [in 4 g + r][out p]; edge register i of lane 4 b + j = [in0 + i][out0 + j].
__device__ __forceinline__ void fold_ce(float* sl, const f32x4& G0, const f32x4& E, const EdgeMap& em, int pq, int gq,
                                        int lane, float* dump) {
  float* dc[4];
  float* de[4];
  float vc[4], ve[4];
  bool ok[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    dc[r] = sl + (4 * gq + r) * kW + pq;
    const int in = em.in0 + r, out = em.out0 + (lane & 3);
    ok[r] = em.live && in <= kW && out < kW;
    de[r] = ok[r] ? sl + in * kW + out : dump;  // padding: the lane's own dump word (branch-free)
    vc[r] = *dc[r];
    ve[r] = *de[r];
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    *dc[r] = vc[r] + G0[r];
    *de[r] = ve[r] + E[r];
  }
}

// One outer-product stream of a width-20 weight gradient, sum over the tile's pairs of av (x) bv (av: the
// layer input, rows = in, plus the constant bias_row at in = 20; bv: rows = out), through the transpose
// images: the 16 x 16 core on 16x16x4, the edge blocks on 4x4x1.
__device__ __forceinline__ void outer_stream(float* tA, float* tB, const float (&bv)[kNS], const float (&av)[kNS],
                                             float bias_row, int pq, int gq, int ppq, float* dump, const EdgeMap& em,
                                             f32x4& G0, f32x4& E) {
  put_slots<kNS>(tA, bv, pq, gq);
  put_slots<kNS>(tB, av, pq, gq);
  *(gq == 0 ? tB + img_at(kW, ppq) : dump) = bias_row;
  const f32x4 fa = get_rows(tA, 0, pq, gq), fb = get_rows(tB, 0, pq, gq);
  f32x4 ea[4], eb[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    ea[q] = *reinterpret_cast<const f32x4*>(tB + img_chunk(em.ra, q));
    eb[q] = *reinterpret_cast<const f32x4*>(tA + img_chunk(em.rb, q));
  }
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) G0 = mfma(fb[ks], fa[ks], G0);
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) E = mfma4(ea[q][ks], eb[q][ks], E);
}

// The wave's private gradient slab (LDS, no atomics: deterministic): slab[qoff + in * pitch + out] +=
// G[ib][ob], the tile of rows in = 16 ib + 4 g + r (in == pin is the bias row), columns out = 16 ob + p.
// Row-major with pitch = 20 / 44 puts lane groups g = 0 / 1 on the two halves of the 32 banks
// (4 pitch = 16 mod 32): conflict-free read-modify-writes. Padding entries go to the lane's own dump word.
template <int IBN, int OBN>
__device__ __forceinline__ void fold(float* slab, int qoff, int pitch, int nout, int pin, const f32x4 (&G)[IBN][OBN],
                                     int p, int g, float* dump) {
  float* dst[IBN][OBN][4];
  float v[IBN][OBN][4];
  bool ok[IBN][OBN][4];
#pragma unroll
  for (int ib = 0; ib < IBN; ++ib)
#pragma unroll
    for (int ob = 0; ob < OBN; ++ob)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int in = 16 * ib + 4 * g + r, out = 16 * ob + p;
        ok[ib][ob][r] = out < nout && in <= pin;
        dst[ib][ob][r] = ok[ib][ob][r] ? slab + qoff + in * pitch + out : dump;
        v[ib][ob][r] = *dst[ib][ob][r];
      }
#pragma unroll
  for (int ib = 0; ib < IBN; ++ib)
#pragma unroll
    for (int ob = 0; ob < OBN; ++ob)
#pragma unroll
      for (int r = 0; r < 4; ++r) *dst[ib][ob][r] = v[ib][ob][r] + G[ib][ob][r];
}

// the four forward streams entering the next layer from a layer's checkpoint (h, z'_u, z'_v, z''_v)
__device__ __forceinline__ void streams_of(const float (&h)[kNS], const float (&zu)[kNS], const float (&zv)[kNS],
                                           const float (&zw)[kNS], float (&H)[4][kNS]) {
#pragma unroll
  for (int k = 0; k < kNS; ++k) {
    const float s1 = 1.f - h[k] * h[k], s2 = -2.f * h[k] * s1;
    H[0][k] = h[k];
    H[1][k] = s1 * zu[k];
    H[2][k] = s1 * zv[k];
    H[3][k] = fmaf(s1, zw[k], s2 * zv[k] * zv[k]);
  }
}
template <int S>
__device__ __forceinline__ void stream_of(const float (&h)[kNS], const float (&zu)[kNS], const float (&zv)[kNS],
                                          const float (&zw)[kNS], float (&H)[kNS]) {
#pragma unroll
  for (int k = 0; k < kNS; ++k) {
    const float s1 = 1.f - h[k] * h[k];
    if constexpr (S == 0) H[k] = h[k];
    else if constexpr (S == 1) H[k] = s1 * zu[k];
    else if constexpr (S == 2) H[k] = s1 * zv[k];
    else H[k] = fmaf(s1, zw[k], -2.f * h[k] * s1 * zv[k] * zv[k]);
  }
}

// -------------------------------------------------------------------------------------------------
// pass 2: d/dtheta of sum_ij l_ij (and the loss slots), 16-pair tiles
// -------------------------------------------------------------------------------------------------
template <int KD>
__global__ __launch_bounds__(kWaves2 * kWave, 1) void kmvq_grad_kernel(Args a) {
  extern __shared__ f32x4 lds4[];
  float* lds = reinterpret_cast<float*>(lds4);
  float* img = lds;
  const int slab_f = (a.P + 3) & ~3;
  const int lane0 = threadIdx.x & (kWave - 1), p = lane0 & 15, g = lane0 >> 4;
  const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  float* slab = lds + a.net.img_floats + wib * slab_f;  // this wave's private gradient slab
  float* tA0 = lds + a.net.img_floats + kWaves2 * slab_f + wib * kTImg;
  float* tB0 = tA0 + kRowsA * kPS;
  float* tA1 = tA0;
  float* tB1 = tB0;
  stage_image(lds4, a.net);
  for (int q = threadIdx.x; q < kWaves2 * (slab_f + kTImg); q += blockDim.x) lds[a.net.img_floats + q] = 0.f;
  __syncthreads();

  const int64_t wave = (int64_t)blockIdx.x * kWaves2 + wib;
  const int64_t n_waves = (int64_t)gridDim.x * kWaves2;
  const int L = a.net.L, D = a.net.D;
  const float c2 = -2.f * a.s;
  float accs[3] = {0.f, 0.f, 0.f};  // LOSS, HESSIAN, FRICTION slot partials
  float cs[kNS] = {}, c0sum = 0.f;   // sum c0 h (the dl/dc remainder), sum c0 (dl/db's |b|^2 term)

  for (int64_t unit = wave; unit < a.n_units; unit += n_waves) {
    const int64_t it = unit / a.n_ch, ch = unit - it * a.n_ch;
    const int64_t t = it / a.n, i = it - t * a.n;
    const int64_t j_end = (ch + 1) * kChunk < a.n ? (ch + 1) * kChunk : a.n;
    const float* zt = a.z + t * a.set_stride;
    float xi[KD], vi[KD], ui[KD];
    lane_dims<KD>(zt + i * a.ld, D, g, xi);
    lane_dims<KD>(zt + i * a.ld + D, D, g, vi);
    lane_dims<KD>(a.gbar + it * D, D, g, ui);
#pragma unroll
    for (int kk = 0; kk < KD; ++kk) ui[kk] *= 2.f * a.s;
    const float dsa = a.ds[it * 2], dsb = a.ds[it * 2 + 1];
    const float c0 = 2.f * a.s * (dsb + dsa * dsa + a.gamma * dsa);  // 2 s w_it (:84-89)

    // layer-0 tangents along u and v: the same for every pair of the item
    float w0[4];
    load_units<4>(img, a.net.fwd[0], lane0, w0);  // unit kk * 2 + mb
    float zu0[kNS], zv0[kNS], zw0[kNS];
    {
      f32x4 Au[2] = {}, Av[2] = {};
#pragma unroll
      for (int kk = 0; kk < KD; ++kk)
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) {
          Au[mb] = mfma(w0[kk * 2 + mb], ui[kk], Au[mb]);
          Av[mb] = mfma(w0[kk * 2 + mb], vi[kk], Av[mb]);
        }
      compact_hidden(Au, zu0);
      compact_hidden(Av, zv0);
#pragma unroll
      for (int k = 0; k < kNS; ++k) zw0[k] = 0.f;
    }

    float xn[KD];  // next tile's reference coordinates (prefetched)
    load_ref<KD>(zt, a.ld, D, g, ch * kChunk + p, j_end, xn);
    for (int64_t j0 = ch * kChunk; j0 < j_end; j0 += 16) {
      // the weight fragments are the same for every tile: an opaque lane index keeps the compiler from
      // hoisting all of them out of the tile loop (hundreds of VGPRs)
      int lane = lane0;
      asm volatile("" : "+v"(lane));
      // (opaque too: every lane-dependent LDS address — hoisted, they held ~150 VGPRs)
      const int pq = lane & 15, gq = lane >> 4, ppq = pos_of(pq);
      float* dump = tB0 + 24 * kPS + lane;  // fold's padding entries: rows 24..26 of image B0 (unread)
      const bool active = j0 + p < j_end;
      float yb[KD];
#pragma unroll
      for (int kk = 0; kk < KD; ++kk) yb[kk] = (active && 4 * kk + gq < D) ? xi[kk] - xn[kk] : 0.f;
      load_ref<KD>(zt, a.ld, D, gq, j0 + 16 + p, j_end, xn);  // under this tile's products
      // ---- forward ----
      float ckh[kLMax][kNS], cku[kLMax][kNS], ckv[kLMax][kNS], ckw[kLMax][kNS];
      float H[4][kNS];
      {
        f32x4 A[2];
        bias_hidden(img, a.net.bias[0], gq, A);
#pragma unroll
        for (int kk = 0; kk < KD; ++kk)
#pragma unroll
          for (int mb = 0; mb < 2; ++mb) A[mb] = mfma(w0[kk * 2 + mb], yb[kk], A[mb]);
        float z[kNS];
        compact_hidden(A, z);
#pragma unroll
        for (int k = 0; k < kNS; ++k) ckh[0][k] = ftanh(z[k]);
        streams_of(ckh[0], zu0, zv0, zw0, H);
      }
#pragma unroll
      for (int l = 1; l < kLMax; ++l) {
        if (l < L) {
          float w[12];
          load_units<12>(img, a.net.fwd[l], lane, w);  // unit kk * 2 + mb
          f32x4 A[4][2] = {};
          bias_hidden(img, a.net.bias[l], gq, A[0]);
#pragma unroll
          for (int s = 0; s < 4; ++s)  // stream-major: the primal's tanh overlaps the tangents' MFMAs
#pragma unroll
            for (int kk = 0; kk < kNS; ++kk)
#pragma unroll
              for (int mb = 0; mb < 2; ++mb) A[s][mb] = mfma(w[kk * 2 + mb], H[s][kk], A[s][mb]);
          float z0[kNS];
          compact_hidden(A[0], z0);
          compact_hidden(A[1], cku[l]);
          compact_hidden(A[2], ckv[l]);
          compact_hidden(A[3], ckw[l]);
#pragma unroll
          for (int k = 0; k < kNS; ++k) ckh[l][k] = ftanh(z0[k]);
          // copied out of the accumulator tuples now (block 1 holds one live value in four registers)
          launder(cku[l]); launder(ckv[l]); launder(ckw[l]); launder(ckh[l]);
          streams_of(ckh[l], cku[l], ckv[l], ckw[l], H);
        }
      }
      // ---- output layer as a quadratic form: Phi = |K_L^T h + b|^2 = dh^T M dh + 2 c0^T dh + |y0|^2 with
      // M = K_L K_L^T (20 x 20), dh = h - h0, c0 = K_L y0, y0 = K_L^T h0 + b (kmvq_h0_kernel,
      // kmvq_image_kernel). The four streams' M-products give every
      // output-side term: T0 = Phi, T2 = v^T Hess Phi v, the adjoints of the four h streams (no backward
      // product through K_L), and dl/dM, dl/dc as two outer products over the pairs (the K_L / b gradient
      // follows once per call, kmvq_out_post_kernel). 40 + 8 + 32 (4x4x1) MFMAs replace 60 + 80 + 96. ----
      float hb[4][kNS];
      {
        // the primal enters the quadratic form shifted by h0 (Phi = dh^T M dh + 2 c0^T dh + |y0|^2 with
        // dh = h - h0, y0 = K_L^T h0 + b, c0 = K_L y0): every term is then O(|y|) where the net's output
        // y is small — pairs near the origin of a trained net, where Phi*(0) = 0 — instead of the
        // difference of O(|b|^2) terms (the unshifted fold's fp32 cancellation)
        const float* h0p = img + a.net.h0_off;
#pragma unroll
        for (int k = 0; k < 4; ++k) H[0][k] -= h0p[4 * gq + k];
        H[0][4] -= h0p[16 + gq];
        float w[12];
        load_units<12>(img, a.net.fwd_out, lane, w);  // M, unit kk * 2 + mb
        f32x4 Mh[4][2] = {};
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int kk = 0; kk < kNS; ++kk)
#pragma unroll
            for (int mb = 0; mb < 2; ++mb) Mh[s][mb] = mfma(w[kk * 2 + mb], H[s][kk], Mh[s][mb]);
        float m[4][kNS], cv[kNS];
#pragma unroll
        for (int s = 0; s < 4; ++s) compact_hidden(Mh[s], m[s]);
        const float* cb = img + a.net.bias_out;  // c0[20], |y0|^2
#pragma unroll
        for (int k = 0; k < 4; ++k) cv[k] = cb[4 * gq + k];
        cv[4] = cb[16 + gq];
        float T0 = gq == 0 ? cb[kW] : 0.f, T2 = 0.f;  // |y0|^2 once per pair (lane group 0)
        float q1[kNS], q2[kNS];
#pragma unroll
        for (int k = 0; k < kNS; ++k) {
          const float m0 = m[0][k] + cv[k];  // M h + c
          T0 = fmaf(H[0][k], m0 + cv[k], T0);
          T2 = fmaf(H[2][k], m[2][k], fmaf(H[0][k], m[3][k], fmaf(cv[k], H[3][k], T2)));
          // l = 2 (h^T M h'_u + c^T h'_u) + c2 T2 + c0 T0
          hb[0][k] = active ? 2.f * m[1][k] + 2.f * c2 * m[3][k] + 2.f * c0 * m0 : 0.f;
          hb[1][k] = active ? 2.f * m0 : 0.f;
          hb[2][k] = active ? 4.f * c2 * m[2][k] : 0.f;
          hb[3][k] = active ? 2.f * c2 * m0 : 0.f;
          // dl/dM = sum h (x) (2 h'_u + 2 c2 h''_v + c0 h) + h'_v (x) 2 c2 h'_v; dl/dc = that first factor
          // summed (the bias row) + c0 sum h (cs, a per-lane accumulator over the whole launch)
          q1[k] = active ? 2.f * H[1][k] + 2.f * c2 * H[3][k] + c0 * H[0][k] : 0.f;
          q2[k] = active ? 2.f * c2 * H[2][k] : 0.f;
          cs[k] += active ? c0 * H[0][k] : 0.f;
        }
        T2 *= 2.f;
        accs[0] += active ? c2 * T2 + c0 * T0 : 0.f;
        accs[1] += active ? -0.5f * c2 * T2 : 0.f;
        accs[2] += active ? c0 * T0 : 0.f;
        c0sum += (active && gq == 0) ? c0 : 0.f;
        const EdgeMap em(lane);
        f32x4 G0 = {}, E = {};
        outer_stream(tA0, tB0, q1, H[0], 1.f, pq, gq, ppq, dump, em, G0, E);
        outer_stream(tA1, tB1, q2, H[2], 0.f, pq, gq, ppq, dump, em, G0, E);
        fold_ce(slab + a.qoff_out, G0, E, em, pq, gq, lane, dump);
      }
      // ---- reverse sweep over the tanh layers ----
      auto zbar_of = [&](const float (&h)[kNS], const float (&zu)[kNS], const float (&zv)[kNS],
                         const float (&zw)[kNS], float (&zb)[4][kNS]) {
#pragma unroll
        for (int k = 0; k < kNS; ++k) {
          const float s1 = 1.f - h[k] * h[k], s2 = -2.f * h[k] * s1, s3 = -2.f * s1 * s1 - 2.f * h[k] * s2;
          const float b0 = hb[0][k], b1 = hb[1][k], b2 = hb[2][k], b3 = hb[3][k];
          zb[3][k] = s1 * b3;
          zb[2][k] = fmaf(s1, b2, 2.f * s2 * zv[k] * b3);
          zb[1][k] = s1 * b1;
          zb[0][k] = fmaf(s1, b0, fmaf(s2, fmaf(zu[k], b1, zv[k] * b2), fmaf(s2, zw[k], s3 * zv[k] * zv[k]) * b3));
        }
      };
#pragma unroll
      for (int l = kLMax - 1; l >= 1; --l) {
        if (l < L) {
          launder(ckh[l]); launder(cku[l]); launder(ckv[l]); launder(ckw[l]);
          launder(ckh[l - 1]);
          if (l - 1 > 0) { launder(cku[l - 1]); launder(ckv[l - 1]); launder(ckw[l - 1]); }
          float zb[4][kNS];
          zbar_of(ckh[l], cku[l], ckv[l], ckw[l], zb);
          const float(&ph)[kNS] = ckh[l - 1];
          const float(&pu)[kNS] = l - 1 == 0 ? zu0 : cku[l - 1];
          const float(&pv)[kNS] = l - 1 == 0 ? zv0 : ckv[l - 1];
          const float(&pw)[kNS] = l - 1 == 0 ? zw0 : ckw[l - 1];
          float w[12];
          load_units<12>(img, a.net.bwd[l], lane, w);  // unit kk * 2 + mb
          f32x4 G0 = {}, E = {}, B[4][2] = {};
          const EdgeMap em(lane);
          auto step = [&](auto sc) {
            constexpr int s = decltype(sc)::value;
            float* tA = s & 1 ? tA1 : tA0;
            float* tB = s & 1 ? tB1 : tB0;
            float Hp[kNS];
            stream_of<s>(ph, pu, pv, pw, Hp);
            put_slots<kNS>(tA, zb[s], pq, gq);
            put_slots<kNS>(tB, Hp, pq, gq);
            *(gq == 0 ? tB + img_at(kW, ppq) : dump) = s == 0 ? 1.f : 0.f;
            const f32x4 fa = get_rows(tA, 0, pq, gq), fb = get_rows(tB, 0, pq, gq);
            f32x4 ea[4], eb[4];  // edge operands: 4 pairs per 16-byte read (pairs q + 4 ks)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              ea[q] = *reinterpret_cast<const f32x4*>(tB + img_chunk(em.ra, q));
              eb[q] = *reinterpret_cast<const f32x4*>(tA + img_chunk(em.rb, q));
            }
            // the backward product of this stream needs no LDS: it covers the images' round trip
#pragma unroll
            for (int kk = 0; kk < kNS; ++kk)
#pragma unroll
              for (int mb = 0; mb < 2; ++mb) B[s][mb] = mfma(w[kk * 2 + mb], zb[s][kk], B[s][mb]);
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) G0 = mfma(fb[ks], fa[ks], G0);
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
              for (int ks = 0; ks < 4; ++ks) E = mfma4(ea[q][ks], eb[q][ks], E);
          };
          step(std::integral_constant<int, 0>{});
          step(std::integral_constant<int, 1>{});
          step(std::integral_constant<int, 2>{});
          step(std::integral_constant<int, 3>{});
          fold_ce(slab + a.qoff[l], G0, E, em, pq, gq, lane, dump);
#pragma unroll
          for (int s = 0; s < 4; ++s) compact_hidden(B[s], hb[s]);
        }
      }
      // layer 0: inputs y (per pair), u, v (per item), 0 (second order)
      {
        launder(ckh[0]); launder(zu0); launder(zv0);
        float zb[4][kNS];
        zbar_of(ckh[0], zu0, zv0, zw0, zb);
        f32x4 G[1][2] = {};
#pragma unroll
        for (int s = 0; s < 3; ++s) {
          float* tA = s & 1 ? tA1 : tA0;
          float* tB = s & 1 ? tB1 : tB0;
          put_slots<kNS>(tA, zb[s], pq, gq);
#pragma unroll
          for (int kk = 0; kk < KD; ++kk) {
            const int k = 4 * kk + gq;  // rows past D go to row 15 (a column no layer-0 output reads)
            tB[img_at(k < D ? k : 15, ppq)] = s == 0 ? yb[kk] : (s == 1 ? ui[kk] : vi[kk]);
          }
          *(gq == 0 ? tB + img_at(D, ppq) : dump) = s == 0 ? 1.f : 0.f;
          f32x4 fa[2], fb;
#pragma unroll
          for (int b = 0; b < 2; ++b) fa[b] = get_rows(tA, b, pq, gq);
          fb = get_rows(tB, 0, pq, gq);
#pragma unroll
          for (int ks = 0; ks < 4; ++ks)
#pragma unroll
            for (int ob = 0; ob < 2; ++ob) G[0][ob] = mfma(fb[ks], fa[ob][ks], G[0][ob]);
        }
        fold<1, 2>(slab, a.qoff[0], kW, kW, D, G, pq, gq, dump);
      }
    }
  }
  float* as = a.aslab + wave * 8;
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const float v = wave_sum(accs[q]);
    if (lane0 == 0) as[q] = v;
  }
  {  // the output region's tail: [21 x 20] | c0 sum h [20] | sum c0
    float* tail = slab + a.qoff_out + (kW + 1) * kW;
#pragma unroll
    for (int k = 0; k < kNS; ++k) {
      float v = cs[k];
#pragma unroll
      for (int off = 8; off > 0; off >>= 1) v += __shfl_xor(v, off, 16);
      if (p == 0) tail[slot_feat(kNS, k, g)] += v;
    }
    const float v = wave_sum(c0sum);
    if (lane0 == 0) tail[kW] += v;
  }
  float* gs = a.gslab + wave * a.P;
  for (int q = lane0; q < a.P; q += kWave) gs[q] = slab[q];
}

// -------------------------------------------------------------------------------------------------
// pair force: the partials per (item, chunk of references), sum_j grad_y Phi(x_i - r_j), and their reduce
// -------------------------------------------------------------------------------------------------
template <int KD>
__global__ __launch_bounds__(kWaves * kWave, 2) void pair_force_kernel(PairForce a) {
  extern __shared__ f32x4 lds4[];
  float* img = reinterpret_cast<float*>(lds4);
  stage_image(lds4, a.net);
  __syncthreads();
  const int lane0 = threadIdx.x & (kWave - 1), p = lane0 & 15, g = lane0 >> 4;
  const int wib = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int64_t wave = (int64_t)blockIdx.x * kWaves + wib;
  const int64_t n_waves = (int64_t)gridDim.x * kWaves;
  const int D = a.net.D;
  const int64_t n_ch = pair_chunks(a.m), n_units = a.n_sets * a.n * n_ch;
  for (int64_t unit = wave; unit < n_units; unit += n_waves) {
    const int64_t it = unit / n_ch, ch = unit - it * n_ch;
    const int64_t t = it / a.n, i = it - t * a.n;
    const int64_t j_end = (ch + 1) * kChunk < a.m ? (ch + 1) * kChunk : a.m;
    const float* rt = a.r + t * a.r_set;
    float xi[KD];
    lane_dims<KD>(a.x + t * a.x_set + i * a.ldx, D, g, xi);
    f32x4 gacc = {};
    float xn[KD];
    load_ref<KD>(rt, a.ldr, D, g, ch * kChunk + p, j_end, xn);
    for (int64_t j0 = ch * kChunk; j0 < j_end; j0 += 16) {
      // the weight fragments are the same for every tile: an opaque lane index keeps the compiler from hoisting
      // all of them out of the tile loop (hundreds of VGPRs)
      int lane = lane0;
      asm volatile("" : "+v"(lane));
      const bool active = j0 + p < j_end;
      float yb[KD];
#pragma unroll
      for (int kk = 0; kk < KD; ++kk) yb[kk] = (active && 4 * kk + g < D) ? xi[kk] - xn[kk] : 0.f;
      load_ref<KD>(rt, a.ldr, D, g, j0 + 16 + p, j_end, xn);  // the next tile's rows, under this tile's products
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

__global__ __launch_bounds__(kBlock) void pair_force_reduce_kernel(const float* __restrict__ gpart, int64_t n_items,
                                                                   int n_ch, int D, double inv_m,
                                                                   float* __restrict__ out) {
  const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (q >= n_items * D) return;
  const int64_t it = q / D;
  out[q] = reduce_chunks(gpart, it, n_ch, D, (int)(q - it * D), inv_m);
}

// -------------------------------------------------------------------------------------------------
// weight image (layout and plan: mlp_tile.h ImageArgs / image_plan)
// -------------------------------------------------------------------------------------------------
constexpr int kOutRegion = (kW + 1) * kW + kW + 4;  // slab of the folded output layer: [21][20] | c0 sum h | sum c0

// h0 = the last tanh layer's output at input 0 and y0 = K_L^T h0 + b (one block): the expansion point of
// the folded output layer (h0y0 = [h0 (W) | y0 (O)], fp64 slots). h0 goes through the pair kernels' own
// fp32 arithmetic (ftanh), so that dh = h(y) - h0 vanishes at y = 0 and the tanh approximation's bias
// cancels in it; any h0 keeps the fold exact (y0 and c0 are formed from the stored h0, in fp64).
__global__ __launch_bounds__(256) void kmvq_h0_kernel(ImageArgs ia, const float* __restrict__ prm,
                                                      double* __restrict__ h0y0) {
  __shared__ float hs[2][kW];
  const int L = ia.L, W = ia.W, O = ia.O, t = threadIdx.x;
  for (int l = 0; l < L; ++l) {
    const int din = l == 0 ? ia.D : W;
    const float* K = prm + ia.roff[l];
    if (t < W) {
      float z = K[(int64_t)din * W + t];  // the bias (layer 0: the input is 0)
      if (l > 0)
        for (int k = 0; k < W; ++k) z = fmaf(hs[(l - 1) & 1][k], K[(int64_t)k * W + t], z);
      hs[l & 1][t] = ftanh(z);
    }
    __syncthreads();
  }
  const float* h0 = hs[(L - 1) & 1];
  const float* KL = prm + ia.roff[L];
  for (int o = t; o < O; o += blockDim.x) {
    double y = (double)KL[(int64_t)W * O + o];
    for (int f = 0; f < W; ++f) y += (double)h0[f] * (double)KL[(int64_t)f * O + o];
    h0y0[W + o] = y;
  }
  if (t < W) h0y0[t] = (double)h0[t];
}

// The image: for each tanh layer l the forward (K_l^T, rows = outputs) and backward (K_l, rows = inputs)
// A-operand fragments and the raw bias vector; for the output layer the fragments of M = K_L K_L^T
// (symmetric: one orientation) and [c = K_L b, |b|^2] in its bias slot (the quadratic-form fold).
__global__ void kmvq_image_kernel(ImageArgs ia, const float* __restrict__ prm, const double* __restrict__ h0y0,
                                  float* __restrict__ img) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= ia.img_floats) return;
  const int L = ia.L, W = ia.W, O = ia.O;
  const float* KL = prm + ia.roff[L];  // [W][O], then b [O]
  const int64_t unit_floats = (int64_t)ia.units_total * 64;
  if (q >= unit_floats) {  // biases (padded raw vectors), zero elsewhere
    float v = 0.f;
    const double* y0 = h0y0 + W;
    if ((int)q >= ia.h0_off && (int)q < ia.h0_off + kW + 4) {
      const int o = (int)q - ia.h0_off;
      img[q] = o < W ? (float)h0y0[o] : 0.f;
      return;
    }
    for (int l = 0; l <= L; ++l) {
      const int o = (int)q - ia.bias_off[l];  // bias_off: absolute float offsets
      if (o < 0 || o >= kW + 4) continue;
      if (l < L) {
        const int din = l == 0 ? ia.D : W;
        v = o < W ? prm[ia.roff[l] + (int64_t)din * W + o] : 0.f;
      } else if (o < W) {  // c0 = K_L y0
        double c = 0.0;
        for (int k = 0; k < O; ++k) c += (double)KL[(int64_t)o * O + k] * y0[k];
        v = (float)c;
      } else if (o == kW) {  // |y0|^2
        double yy = 0.0;
        for (int k = 0; k < O; ++k) yy += y0[k] * y0[k];
        v = (float)yy;
      }
      break;
    }
    img[q] = v;
    return;
  }
  const int u = (int)(q / 256), lane = (int)((q / 4) % 64), uu = 4 * u + (int)(q % 4);
  float v = 0.f;
  for (int s = 0; s < ia.nsec; ++s) {
    const int lu = uu - ia.sec_u0[s];
    if (lu < 0 || lu >= ia.sec_units[s]) continue;
    const int l = ia.sec_layer[s], MB = ia.sec_mb[s];
    const int kk = lu / MB, mb = lu % MB;
    const int g = lane >> 4, m = lane & 15;
    const int din = l == 0 ? ia.D : W;
    int in, out;
    if (!ia.sec_bwd[s]) {  // forward: A[m = out row][k = in slot]
      in = l == 0 ? 4 * kk + g : slot_feat(kNS, kk, g);
      out = row_feat(kNS, mb, m);
    } else {  // backward: A[m = in row][k = out slot]
      in = l == 0 ? m : row_feat(kNS, mb, m);
      out = slot_feat(kNS, kk, g);
    }
    if (l == L) {  // M[in][out] = sum_k K_L[in][k] K_L[out][k]
      if (in >= 0 && in < W && out >= 0 && out < W) {
        float mm = 0.f;
        for (int k = 0; k < O; ++k) mm = fmaf(KL[(int64_t)in * O + k], KL[(int64_t)out * O + k], mm);
        v = mm;
      }
    } else if (in >= 0 && in < din && out >= 0 && out < W) {
      v = prm[ia.roff[l] + (int64_t)in * W + out];
    }
    break;
  }
  img[q] = v;
}

// grad[real(q)] += sum_w slab[w][q] (fixed order, fp64) for the tanh layers; loss slots from the
// per-wave partials. The folded output layer's region is reduced by kmvq_out_post_kernel.
__global__ void kmvq_reduce_kernel(MlpPadMap pm, const float* __restrict__ gslab, int n_slabs, int64_t P,
                                   const float* __restrict__ aslab, int64_t n_waves, float* __restrict__ grad,
                                   double* __restrict__ acc) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q < P) {
    const int64_t r = pm.real_of(q);
    if (r >= 0) {
      double s = 0.0;
      for (int b = 0; b < n_slabs; ++b) s += (double)gslab[(int64_t)b * P + q];
      grad[r] += (float)s;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < 3) {
    double s = 0.0;
    for (int64_t w = 0; w < n_waves; ++w) s += (double)aslab[w * 8 + threadIdx.x];
    const int slot = threadIdx.x == 0 ? PDEINV_GMM_ACC_LOSS
                                      : (threadIdx.x == 1 ? PDEINV_GMM_ACC_HESSIAN : PDEINV_GMM_ACC_FRICTION);
    acc[slot] += s;
  }
}

// Output layer from the folded sums (fixed order, fp64): with G_M = dl/dM, G_c = dl/dc0, C0 = sum c0 (the
// weight of |y0|^2), and c0 = K_L y0, y0 = K_L^T h0 + b, M = K_L K_L^T:
//   dl/dK_L = (G_M + G_M^T) K_L + G_c y0^T + h0 (K_L^T G_c)^T + 2 C0 h0 y0^T,
//   dl/db   = K_L^T G_c + 2 C0 y0                                  (h0 = 0: the unshifted fold)
__global__ __launch_bounds__(256) void kmvq_out_post_kernel(const float* __restrict__ gslab, int n_slabs, int64_t P,
                                                            int qoff, int W, int O, const float* __restrict__ KL,
                                                            const double* __restrict__ h0y0, float* __restrict__ gL) {
  __shared__ double red[kOutRegion];
  extern __shared__ double ktg[];  // K_L^T G_c [O]
  for (int e = threadIdx.x; e < kOutRegion; e += blockDim.x) {
    double s = 0.0;
    for (int b = 0; b < n_slabs; ++b) s += (double)gslab[(int64_t)b * P + qoff + e];
    red[e] = s;
  }
  __syncthreads();
  const double* GM = red;                      // [20][20]
  const double* Gc1 = red + kW * kW;           // bias row: sum (2 h'_u + 2 c2 h''_v + c0 h)
  const double* Gc2 = red + (kW + 1) * kW;     // c0 sum h
  const double C0 = red[(kW + 1) * kW + kW];
  const double* h0 = h0y0;
  const double* y0 = h0y0 + W;
  for (int o = threadIdx.x; o < O; o += blockDim.x) {
    double s = 0.0;
    for (int f = 0; f < W; ++f) s += (double)KL[(int64_t)f * O + o] * (Gc1[f] + Gc2[f]);
    ktg[o] = s;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < W * O; e += blockDim.x) {
    const int f = e / O, o = e - f * O;
    double s = (Gc1[f] + Gc2[f]) * y0[o] + h0[f] * (ktg[o] + 2.0 * C0 * y0[o]);
    for (int f2 = 0; f2 < W; ++f2) s += (GM[f * kW + f2] + GM[f2 * kW + f]) * (double)KL[(int64_t)f2 * O + o];
    gL[e] += (float)s;
  }
  for (int o = threadIdx.x; o < O; o += blockDim.x) gL[(int64_t)W * O + o] += (float)(ktg[o] + 2.0 * C0 * y0[o]);
}

int build_image(const ImageArgs& ia, const float* params, double* h0y0, float* img, hipStream_t st) {
  hipLaunchKernelGGL(kmvq_h0_kernel, dim3(1), dim3(256), 0, st, ia, params, h0y0);
  hipLaunchKernelGGL(kmvq_image_kernel, dim3((unsigned)((ia.img_floats + 255) / 256)), dim3(256), 0, st, ia, params,
                     (const double*)h0y0, img);
  return check_launch("kmvq_image_kernel");
}

int device_cus() {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
    cus = 256;
  return cus;
}

int pair_force_partials(const PairForce& f, hipStream_t st) {
  const int64_t n_units = f.n_sets * f.n * pair_chunks(f.m);
  if (n_units <= 0) return PDEINV_OK;
  const int64_t need = (n_units + kWaves - 1) / kWaves, cap = 2 * (int64_t)device_cus();
  const dim3 gr((unsigned)(need < cap ? need : cap)), bl(kWaves * kWave);
  const size_t lds = sizeof(float) * (size_t)f.net.img_floats;
  if (f.net.D <= 4) {
    allow_lds(pair_force_kernel<1>);
    hipLaunchKernelGGL(pair_force_kernel<1>, gr, bl, lds, st, f);
  } else {
    allow_lds(pair_force_kernel<2>);
    hipLaunchKernelGGL(pair_force_kernel<2>, gr, bl, lds, st, f);
  }
  return check_launch("pair_force_kernel");
}

int pair_force_reduce(const float* gpart, int64_t n_items, int n_ch, int D, double inv_m, float* out,
                      hipStream_t st) {
  const int64_t nq = n_items * D;
  if (nq <= 0) return PDEINV_OK;
  hipLaunchKernelGGL(pair_force_reduce_kernel, dim3((unsigned)((nq + kBlock - 1) / kBlock)), dim3(kBlock), 0, st,
                     gpart, n_items, n_ch, D, inv_m, out);
  return check_launch("pair_force_reduce_kernel");
}

}  // namespace mlpq

// ---- host driver of the residual ---------------------------------------------------------------
namespace {

struct QPlan {
  mlpq::ImagePlan ip;
  MlpPadMap pm;
  int n_ch, n_blocks2;
  int64_t items, n_units, P;
  size_t lds2;                                                               // bytes
  size_t off_img, off_gbar, off_gpart, off_gslab, off_aslab, off_h0, total;  // bytes
};

QPlan q_plan(const pdeinv_kmv_mlp_desc* d) {
  QPlan p{};
  const int L = d->n_layers;
  p.ip = mlpq::image_plan(d->dim, L, d->width, d->out_features);
  const mlpq::ImageArgs& ia = p.ip.ia;
  // padded parameter layout of the gradient slab: K [pin][20] then b [20] for the tanh layers (row
  // pitch 20: 4 pitch = 16 mod 32), then the folded output layer's region (kOutRegion floats). The
  // pad map covers the tanh layers only (pm.L = L - 1); the output region goes through kmvq_out_post_kernel.
  p.pm.L = L - 1;
  int64_t ro = 0, po = 0;
  for (int l = 0; l <= L; ++l) {
    const int din = l == 0 ? d->dim : d->width, dout = l == L ? d->out_features : d->width;
    p.pm.roff[l] = ro;  // = ia.roff[l]
    p.pm.poff[l] = po;
    if (l < L) {  // rows: layer 0 its D inputs, the others the padded width (the kernels' bias row is 20)
      const int pin = l == 0 ? d->dim : mlpq::kW;
      p.pm.din[l] = din;
      p.pm.dout[l] = dout;
      p.pm.pin[l] = pin;
      p.pm.pout[l] = mlpq::kW;
      po += (int64_t)pin * mlpq::kW + mlpq::kW;
    } else {
      po += mlpq::kOutRegion;
    }
    ro += (int64_t)din * dout + dout;
  }
  p.P = po;
  p.items = (int64_t)d->n_sets * d->n_rows;
  p.n_ch = mlpq::pair_chunks(d->n_rows);
  p.n_units = p.items * p.n_ch;
  const int cus = mlpq::device_cus();
  const int64_t need2 = (p.n_units + mlpq::kWaves2 - 1) / mlpq::kWaves2;
  p.n_blocks2 = (int)(need2 < cus ? need2 : cus);
  p.lds2 = sizeof(float) * ((size_t)ia.img_floats +
                            (size_t)mlpq::kWaves2 * ((((size_t)p.P + 3) & ~(size_t)3) + mlpq::kTImg));
  using mlpq::take;
  p.off_img = take(p.total, sizeof(float) * (size_t)ia.img_floats);
  p.off_gbar = take(p.total, sizeof(float) * (size_t)p.items * d->dim);
  p.off_gpart = take(p.total, sizeof(float) * (size_t)p.n_units * d->dim);
  p.off_gslab = take(p.total, sizeof(float) * (size_t)cus * mlpq::kWaves2 * p.P);
  p.off_aslab = take(p.total, sizeof(float) * (size_t)cus * mlpq::kWaves2 * 8);
  p.off_h0 = take(p.total, sizeof(double) * (size_t)(d->width + d->out_features));
  return p;
}

template <int KD>
int launch_grad(const mlpq::Args& a, const QPlan& p, hipStream_t st) {
  mlpq::allow_lds(mlpq::kmvq_grad_kernel<KD>);
  hipLaunchKernelGGL((mlpq::kmvq_grad_kernel<KD>), dim3((unsigned)p.n_blocks2), dim3(mlpq::kWaves2 * kWave), p.lds2,
                     st, a);
  return check_launch("kmvq_grad_kernel");
}

}  // namespace

bool kmvq_supported(const pdeinv_kmv_mlp_desc* d) {
  if (d->impl == PDEINV_MLP_IMPL_PAIRS_RING) return false;  // explicit A/B selection of the register-ring kernels
  return mlpq::tile_envelope(d->dim, d->n_layers, d->width, d->out_features) && q_plan(d).lds2 <= mlpq::kLdsMax;
}

size_t kmvq_workspace_bytes(const pdeinv_kmv_mlp_desc* d) { return q_plan(d).total; }

// pass 0: weight image + gbar (returned through gbar_out); pass 1: the gradient (grad, acc accumulate +=)
int kmvq_run(const pdeinv_kmv_mlp_desc* d, const float* z, int64_t set_stride, int64_t ld, const float* ds,
             const float* params, void* ws, double* acc, float* grad, float** gbar_out, int pass, hipStream_t st) {
  const QPlan p = q_plan(d);
  char* w = (char*)ws;
  float* img = (float*)(w + p.off_img);
  float* gbar = (float*)(w + p.off_gbar);
  double* h0y0 = (double*)(w + p.off_h0);
  if (gbar_out) *gbar_out = gbar;
  const int L = d->n_layers;
  if (pass == 0) {  // gbar_i = mean_j grad Phi(x_i - x_j) within each time stamp
    int rc = mlpq::build_image(p.ip.ia, params, h0y0, img, st);
    if (rc) return rc;
    mlpq::PairForce f{};
    f.x = f.r = z;
    f.ldx = f.ldr = ld;
    f.x_set = f.r_set = set_stride;
    f.n_sets = d->n_sets;
    f.n = f.m = d->n_rows;
    f.gpart = (float*)(w + p.off_gpart);
    f.net = mlpq::tile_net(p.ip, img);
    rc = mlpq::pair_force_partials(f, st);
    if (rc) return rc;
    return mlpq::pair_force_reduce(f.gpart, p.items, p.n_ch, d->dim, 1.0 / (double)d->n_rows, gbar, st);
  }
  mlpq::Args a{};
  a.n_ch = p.n_ch;
  a.n = d->n_rows;
  a.n_units = p.n_units;
  a.set_stride = set_stride;
  a.ld = ld;
  a.z = z;
  a.ds = ds;
  a.gamma = d->gamma;
  a.s = (float)(1.0 / ((double)d->n_rows * (double)d->n_rows * (double)d->n_sets));
  a.net = mlpq::tile_net(p.ip, img);
  for (int l = 0; l <= L; ++l) a.qoff[l] = (int)p.pm.poff[l];
  a.qoff_out = (int)p.pm.poff[L];
  a.P = (int)p.P;
  a.gbar = gbar;
  a.gslab = (float*)(w + p.off_gslab);
  a.aslab = (float*)(w + p.off_aslab);
  int rc = p.ip.KD == 1 ? launch_grad<1>(a, p, st) : launch_grad<2>(a, p, st);
  if (rc) return rc;
  const int n_slabs = p.n_blocks2 * mlpq::kWaves2;
  hipLaunchKernelGGL(mlpq::kmvq_reduce_kernel, dim3((unsigned)((p.P + 255) / 256)), dim3(256), 0, st, p.pm, a.gslab,
                     n_slabs, p.P, a.aslab, (int64_t)n_slabs, grad, acc);
  rc = check_launch("kmvq_reduce_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(mlpq::kmvq_out_post_kernel, dim3(1), dim3(256), sizeof(double) * (size_t)d->out_features, st,
                     a.gslab, n_slabs, p.P, a.qoff_out, d->width, d->out_features, params + p.ip.ia.roff[L],
                     (const double*)h0y0, grad + p.ip.ia.roff[L]);
  return check_launch("kmvq_out_post_kernel");
}

}  // namespace pdeinv
