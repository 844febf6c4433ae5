// The operator on device tensors: out = alpha (A + sigma I) x + beta x + gamma y + c0 on a block of a
// global row-major fp64 array (row stride ld elements, unit column stride), the layout of io_kernels.hip.
//
//   k_apply   interior nodes of the block get the combination, box-boundary nodes of the block get 0.
//             A + sigma I is the plain matrix on the whole box (fictitious region included, no ellipse
//             mask); x counts as 0 on the box boundary and is never loaded there, so whatever the tensor
//             holds on its boundary lines (a NaN included) cannot reach out.
//
// A streaming stencil: lanes run along a row, a workgroup owns kApplyCols columns and marches kApplyRows
// rows top to bottom in steps of kApplyUnroll rows.  Every lane keeps rows i-1, i, i+1 of its column in
// registers, so a row of x is loaded once per tile (plus the tile's two halo rows); the j-1 / j+1
// neighbours come from the neighbouring lanes by DPP wave shifts, and only the first and the last lane of
// a wave load the column next to their wave (one masked load per row).  All lanes stay active for the
// whole kernel (the shifts read every lane): a lane past the block's last column carries the values of
// its own column -- a valid neighbour for the lane before it -- and only its store is masked.  A step
// issues the loads of all its rows before its first store.  Loads of positions outside the interior are
// redirected to the nearest interior node and replaced by 0 afterwards (a select, never a product), so
// no load depends on a branch.  ld = N + 1 is odd in general: every access is one element per lane.
// Stores are ordinary ones: the next reader is usually the caller.
//
// Faces from the 1-D tables as k_init forms them (load_col, load_row, face_a, face_b); a(i+1, j) of one
// row is a(i, j) of the next, bitwise, and is carried over.  (A x) is apply_a<true>, the reference's
// operation order without contraction; sigma enters as ONE fma on top, as apply_a_sh.
//
// SH = 2 (a session with a reaction field): the shift of a node is read from the shift field T(sigma + c) of
// the subdomain that owns the launch's block (ApplyCoef::shift, its pitch and local origin) with the step's
// other loads, and enters in sigma's place -- so apply, the solver and residual_norm share one operator,
// for fp32 storage too.  SH = 0 / 1 are the kernels they were.
//
// SH = 3 (a session with a diffusion field): as 2, and the faces of a node come from the owning subdomain's
// face-coefficient fields (ApplyCoef::ka / kb, the shift field's layout) with the step's other loads: ak of
// the next row (carried over like the table value), bk of the node and of the column after it.
#include <cmath>
#include <cstdint>
#include <type_traits>

#include "pcg_device.hpp"
#include "pmx/common.hpp"
#include "pmx/kernels.hpp"

namespace pmx {

using namespace dev;

namespace {

constexpr int kApplyCols = 256;   // threads per workgroup, one column each
constexpr int kApplyRows = 32;    // rows a workgroup marches
constexpr int kApplyUnroll = 8;   // rows per step (loads of a step in flight together)
static_assert(kApplyCols % kWave == 0 && kApplyRows % kApplyUnroll == 0, "whole waves, whole steps");

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// v = alpha Lx; v = fma(beta, xc, v); v = fma(gamma, yc, v) with y; v += c0 -- or Lx itself (plain)
template <bool HAS_Y>
__device__ __forceinline__ double combine(const ApplyCoef& K, double Lx, double xc, double yc) {
  PMX_NO_CONTRACT
  if (K.plain) return Lx;
  double v = K.alpha * Lx;
  v = __builtin_fma(K.beta, xc, v);
  if constexpr (HAS_Y) v = __builtin_fma(K.gamma, yc, v);
  return v + K.c0;
}

}  // namespace

// block: global rows gi_lo .. gi_lo + rows - 1, columns gj_lo .. gj_lo + cols - 1, inside [0, M] x [0, N]
template <int SH, bool HAS_Y, typename T = double>
__global__ void __launch_bounds__(kApplyCols)
k_apply(DevGeom G, DevTables Tb, const double* __restrict__ x, int64_t ldx, const double* y, int64_t ldy,
        double* out, int64_t ldo, int gi_lo, int gj_lo, int rows, int cols, ApplyCoef K) {
  const int M = G.M, N = G.N;
  const int lane = threadIdx.x % kWave;
  const int c = blockIdx.x * kApplyCols + threadIdx.x;
  const int gj = gj_lo + c;  // may lie past the block, or past N
  const int r0 = blockIdx.y * kApplyRows;
  const int rend = min(r0 + kApplyRows, rows);
  const bool jin = gj > 0 && gj < N;
  const int gjc = clampi(gj, 1, N - 1);
  // the column next to the wave: j - 1 for its first lane, j + 1 for its last
  const bool edge = lane == 0 || lane == kWave - 1;
  const int gje = lane == 0 ? gj - 1 : gj + 1;
  const bool ein = gje > 0 && gje < N;
  const int gjec = clampi(gje, 1, N - 1);
  const bool owned = c < cols;
  const int gjs = min(gj, gj_lo + cols - 1);  // y and out: a column of the block for every lane
  const int gi_last = gi_lo + rows - 1;
  const ColConst cc = load_col(Tb, gjc);

  // SH 3: the lane's column of the face fields -- a column of the block and of the interior, so every lane
  // reads cells the setup kernel wrote; rows clamp to the block's (local 0 .. nx+1, +1 for the next row's ak)
  [[maybe_unused]] const int gjk = clampi(gjs, 1, N - 1);
  [[maybe_unused]] const T* fka = static_cast<const T*>(K.ka);
  [[maybe_unused]] const T* fkb = static_cast<const T*>(K.kb);
  [[maybe_unused]] auto kat = [&](int gi) { return int64_t(gi - K.sgi0) * K.spitch + (gjk - K.sgj0); };

  auto rowin = [&](int gi) { return gi > 0 && gi < M; };
  auto xptr = [&](int gi, int j) { return x + int64_t(clampi(gi, 1, M - 1)) * ldx + j; };

  const int gi0 = gi_lo + r0;
  double xm, xc, ec = 0.0;
  {
    const double vm = *xptr(gi0 - 1, gjc), vc = *xptr(gi0, gjc);
    double ve = 0.0;
    if (edge) ve = *xptr(gi0, gjec);
    xm = jin && rowin(gi0 - 1) ? vm : 0.0;
    xc = jin && rowin(gi0) ? vc : 0.0;
    ec = ein && rowin(gi0) ? ve : 0.0;
  }
  // the row tables cover gi = 0 .. M + 1: every row of the block, and the one after it, has an entry
  double a0;
  if constexpr (SH == 3) a0 = double(fka[kat(min(gi0, gi_last))]);
  else a0 = face_a(cc, load_row(Tb, gi0).rv0, G);

  for (int rb = r0; rb < rend; rb += kApplyUnroll) {
    double xp[kApplyUnroll], ep[kApplyUnroll], yv[kApplyUnroll];
    [[maybe_unused]] T sv[kApplyUnroll];
    // the step's loads: rows rb + 1 .. rb + U of x (centre and edge column), rows rb .. rb + U - 1 of y
#pragma unroll
    for (int u = 0; u < kApplyUnroll; ++u) xp[u] = *xptr(gi_lo + rb + u + 1, gjc);
    if constexpr (HAS_Y) {
#pragma unroll
      for (int u = 0; u < kApplyUnroll; ++u) yv[u] = y[int64_t(min(gi_lo + rb + u, gi_last)) * ldy + gjs];
    }
    [[maybe_unused]] T av[kApplyUnroll], bv0[kApplyUnroll], bv1[kApplyUnroll];
    if constexpr (SH == 3) {
#pragma unroll
      for (int u = 0; u < kApplyUnroll; ++u) {
        const int64_t o = kat(min(gi_lo + rb + u, gi_last));
        av[u] = fka[o + K.spitch];
        bv0[u] = fkb[o];
        bv1[u] = fkb[o + 1];
      }
    }
    if constexpr (SH >= 2) {  // local (gi - sgi0, gj - sgj0) of the owning subdomain: its nodes and boundary lines
      const T* sh = static_cast<const T*>(K.shift);
#pragma unroll
      for (int u = 0; u < kApplyUnroll; ++u)
        sv[u] = sh[int64_t(min(gi_lo + rb + u, gi_last) - K.sgi0) * K.spitch + (gjs - K.sgj0)];
    }
#pragma unroll
    for (int u = 0; u < kApplyUnroll; ++u) ep[u] = 0.0;
    if (edge) {
#pragma unroll
      for (int u = 0; u < kApplyUnroll; ++u) ep[u] = *xptr(gi_lo + rb + u + 1, gjec);
    }
#pragma unroll
    for (int u = 0; u < kApplyUnroll; ++u) {
      const int gi = gi_lo + rb + u;  // wave-uniform
      if (rb + u >= rend) break;
      const double xn = jin && rowin(gi + 1) ? xp[u] : 0.0;
      const double en = ein && rowin(gi + 1) ? ep[u] : 0.0;
      const double xjm = dpp_shift<kWaveShr1>(xc, ec), xjp = dpp_shift<kWaveShl1>(xc, ec);
      double a1, b0, b1;
      if constexpr (SH == 3) {
        a1 = double(av[u]); b0 = double(bv0[u]); b1 = double(bv1[u]);
      } else {
        const RowConst rc = load_row(Tb, gi);
        a1 = face_a(cc, rc.rv1, G);
        b0 = face_b(rc, cc.rh0, G); b1 = face_b(rc, cc.rh1, G);
      }
      double Lx = apply_a<true>(xc, xm, xn, xjm, xjp, a0, a1, b0, b1, G);
      if constexpr (SH >= 2) Lx = __builtin_fma(double(sv[u]), xc, Lx);
      else if constexpr (SH == 1) Lx = __builtin_fma(K.sigma, xc, Lx);  // as apply_a_sh
      const double v = jin && rowin(gi) ? combine<HAS_Y>(K, Lx, xc, HAS_Y ? yv[u] : 0.0) : 0.0;
      if (owned) out[int64_t(gi) * ldo + gjs] = v;
      xm = xc;
      xc = xn;
      ec = en;
      a0 = a1;
    }
  }
}

void launch_apply(const DevGeom& G, const DevTables& Tb, const double* x, int64_t ldx, const double* y, int64_t ldy,
                  double* out, int64_t ldo, int gi_lo, int gj_lo, int rows, int cols, const ApplyCoef& K,
                  hipStream_t s) {
  PMX_CHECK(rows > 0 && cols > 0, "empty block");
  PMX_CHECK(G.M >= 2 && G.N >= 2 && gi_lo >= 0 && gj_lo >= 0 && gi_lo + rows <= G.M + 1 && gj_lo + cols <= G.N + 1,
            "k_apply: block (" << gi_lo << ", " << gj_lo << ") + " << rows << " x " << cols << " outside the grid");
  PMX_CHECK(x && out && ldx >= G.N + 1 && ldo >= G.N + 1 && (!y || ldy >= G.N + 1), "k_apply: row stride below N + 1");
  const int64_t gy = (int64_t(rows) + kApplyRows - 1) / kApplyRows;
  PMX_CHECK(gy <= 65535, "too many rows for one launch: " << rows);
  const dim3 grid(unsigned((cols + kApplyCols - 1) / kApplyCols), unsigned(gy)), block(kApplyCols);
  PMX_CHECK(!K.shift || K.selem == 8 || K.selem == 4, "k_apply: the shift and face fields are fp64 or fp32");
  // k_apply<SH, HAS_Y, T>: T is the storage type of the fields, double for the kinds that read none
  with_op_kind(OperatorData<void>{K.sigma, K.shift, K.ka, K.kb}.kind(), [&](auto sh) {
    constexpr int SH = int(decltype(sh)::value);
    auto launch = [&](auto t, auto has_y) {
      hipLaunchKernelGGL((k_apply<SH, decltype(has_y)::value, decltype(t)>), grid, block, 0, s, G, Tb, x, ldx, y, ldy, out,
                         ldo, gi_lo, gj_lo, rows, cols, K);
    };
    auto with_y = [&](auto t) { y ? launch(t, std::true_type{}) : launch(t, std::false_type{}); };
    if constexpr (SH >= 2) {
      if (K.selem == 8) return with_y(double{});
      return with_y(float{});
    }
    with_y(double{});
  });
  HIP_CHECK(hipGetLastError());
}

}  // namespace pmx
