// Device-resident user data: a global row-major fp64 array (row stride ld elements, unit column
// stride) <-> the per-subdomain pitched fields, without a staging buffer on either side.
//
//   k_scatter  a block of the global array -> a field (or any pitched T buffer), rounded to the storage
//              type as the host path's round_to_storage: copied for double, static_cast for float
//   k_finite   raises a flag on any non-finite value of the whole array
//   k_diffusion_check / k_face_fields   a diffusion field: the check of its values, and the two complete
//              face-coefficient fields of a subdomain (geometry and k folded in) from the nodal values
//   k_domain_fields   a level-set domain: the same two fields with the geometric factor from the nodal level-set
//              values (geometry.hpp's ls_* functions), and the right-hand-side mask of the owned nodes
//   k_gather   w of one subdomain, pending steps applied as GpuSubdomainSolver::download_w applies them,
//              -> its block of the global array; global boundary nodes are written as zero
//
// Plain streaming kernels.  Lanes run along a row, a workgroup covers kIoCols columns of kIoRows rows
// and issues its row loads before the first store.  ld = N + 1 is odd in general, so a row of the
// global array starts at any 8-B boundary and the fields' rows are entered at column 1: every access
// is one element per lane (8 B, 4 B for fp32 fields), coalesced, and nothing wider is attempted.
// Stores to the fields are non-temporal like the sweeps' (the next reader is another kernel).
#include <cstdint>

#include "pcg_device.hpp"
#include "pmx/common.hpp"
#include "pmx/geometry.hpp"
#include "pmx/kernels.hpp"

namespace pmx {

namespace {

constexpr int kIoCols = 256;  // threads per workgroup, one column each
constexpr int kIoRows = 8;    // rows per workgroup

dim3 io_grid(int rows, int cols) {
  PMX_CHECK(rows > 0 && cols > 0, "empty block");
  const int64_t gy = (int64_t(rows) + kIoRows - 1) / kIoRows;
  PMX_CHECK(gy <= 65535, "too many rows for one launch: " << rows);
  return dim3(unsigned((cols + kIoCols - 1) / kIoCols), unsigned(gy));
}

}  // namespace

template <typename T>
__global__ void __launch_bounds__(kIoCols)
k_scatter(const double* __restrict__ src, int64_t ld, T* __restrict__ dst, int64_t pitch, int rows, int cols) {
  const int j = blockIdx.x * kIoCols + threadIdx.x;
  const int i0 = blockIdx.y * kIoRows;
  if (j >= cols) return;
  double v[kIoRows] = {};
#pragma unroll
  for (int u = 0; u < kIoRows; ++u)
    if (i0 + u < rows) v[u] = src[int64_t(i0 + u) * ld + j];
#pragma unroll
  for (int u = 0; u < kIoRows; ++u)
    if (i0 + u < rows) __builtin_nontemporal_store(static_cast<T>(v[u]), dst + int64_t(i0 + u) * pitch + j);
}

__global__ void __launch_bounds__(kIoCols)
k_finite(const double* __restrict__ src, int64_t ld, int rows, int cols, int* flag) {
  const int j = blockIdx.x * kIoCols + threadIdx.x;
  const int i0 = blockIdx.y * kIoRows;
  if (j >= cols) return;
  constexpr unsigned long long kExp = 0x7ff0000000000000ull;  // all ones: inf or NaN
  bool bad = false;
#pragma unroll
  for (int u = 0; u < kIoRows; ++u)
    if (i0 + u < rows)
      bad |= (static_cast<unsigned long long>(__double_as_longlong(src[int64_t(i0 + u) * ld + j])) & kExp) == kExp;
  if (bad) *flag = 1;  // every writer stores the same value
}

// k_scatter for a reaction field: dst = T(sigma + c), the sum in fp64 and rounded once to the storage type
template <typename T>
__global__ void __launch_bounds__(kIoCols)
k_scatter_shift(const double* __restrict__ src, int64_t ld, T* __restrict__ dst, int64_t pitch, int rows, int cols,
                double sigma) {
  const int j = blockIdx.x * kIoCols + threadIdx.x;
  const int i0 = blockIdx.y * kIoRows;
  if (j >= cols) return;
  double v[kIoRows] = {};
#pragma unroll
  for (int u = 0; u < kIoRows; ++u)
    if (i0 + u < rows) v[u] = src[int64_t(i0 + u) * ld + j];
#pragma unroll
  for (int u = 0; u < kIoRows; ++u)
    if (i0 + u < rows)
      __builtin_nontemporal_store(static_cast<T>(sigma + v[u]), dst + int64_t(i0 + u) * pitch + j);
}

// k_finite for a reaction field: raises the flag on a NaN, an infinity or a negative value (-0.0 passes)
__global__ void __launch_bounds__(kIoCols)
k_reaction_check(const double* __restrict__ src, int64_t ld, int rows, int cols, int* flag) {
  const int j = blockIdx.x * kIoCols + threadIdx.x;
  const int i0 = blockIdx.y * kIoRows;
  if (j >= cols) return;
  bool bad = false;
#pragma unroll
  for (int u = 0; u < kIoRows; ++u)
    if (i0 + u < rows) {
      const double v = src[int64_t(i0 + u) * ld + j];
      bad |= !(v >= 0.0) || v == __builtin_huge_val();  // !(v >= 0): a NaN or a negative value
    }
  if (bad) *flag = 1;  // every writer stores the same value
}

// k_finite for a diffusion field: raises the flag on a NaN, an infinity or a value <= 0
__global__ void __launch_bounds__(kIoCols)
k_diffusion_check(const double* __restrict__ src, int64_t ld, int rows, int cols, int* flag) {
  const int j = blockIdx.x * kIoCols + threadIdx.x;
  const int i0 = blockIdx.y * kIoRows;
  if (j >= cols) return;
  bool bad = false;
#pragma unroll
  for (int u = 0; u < kIoRows; ++u)
    if (i0 + u < rows) {
      const double v = src[int64_t(i0 + u) * ld + j];
      bad |= !(v > 0.0) || v == __builtin_huge_val();  // !(v > 0): a NaN, a zero or a negative value
    }
  if (bad) *flag = 1;  // every writer stores the same value
}

// The face-coefficient fields of a diffusion session (launch_face_fields): one thread per local cell, rows
// -1 .. nx+3 (the last one of ak alone), every column of the row (-1 .. pitch-2).  The geometric factor is the
// exact formula the s-step's face fields use (coef_a / coef_b), the mean of k and the product in fp64 in the
// order (0.5 (k' + k)) a, rounded once to T.  A face that does not join two nodes of the box gets 1: such
// cells only ever meet masked values, but D of a masked node must not be 0.
template <typename T>
__global__ void __launch_bounds__(kIoCols)
k_face_fields(DevGeom G, DevTables Tb, const double* __restrict__ k, int64_t ld, T* __restrict__ ak, T* __restrict__ bk) {
  using namespace dev;
  const int lj = -1 + int(blockIdx.x * kIoCols + threadIdx.x);
  const int li = -1 + int(blockIdx.y);
  if (lj > int(G.pitch) - 2 || li > G.nx + 3) return;
  const int gi = G.gi0 + li, gj = G.gj0 + lj;
  const bool node = gi >= 0 && gi <= G.M && gj >= 0 && gj <= G.N;
  double a = 1.0, b = 1.0;
  if (node) {
    const double kc = k[int64_t(gi) * ld + gj];
    if (gi >= 1) a = (0.5 * (k[int64_t(gi - 1) * ld + gj] + kc)) * coef_a(Tb, G, gi, gj);
    if (gj >= 1) b = (0.5 * (k[int64_t(gi) * ld + gj - 1] + kc)) * coef_b(Tb, G, gi, gj);
  }
  const int64_t o = int64_t(li) * G.pitch + lj;
  ak[o] = static_cast<T>(a);
  if (li <= G.nx + 2) bk[o] = static_cast<T>(b);
}

// k_face_fields for a level-set domain (launch_domain_fields): the same cells, the same order (0.5 (k' + k)) a and
// the same single rounding; the geometric factor is geo::ls_coef_a / ls_coef_b of phi, the host's functions, which
// return 1 for a face the interior stencils do not read and read phi on nodes of the box only.  k may be null
// (k = 1).  The thread of an owned node also stores its byte of the right-hand-side mask, phi < 0.
template <typename T>
__global__ void __launch_bounds__(kIoCols)
k_domain_fields(DevGeom G, const double* __restrict__ phi, int64_t ldp, const double* __restrict__ k, int64_t ld,
                T* __restrict__ ak, T* __restrict__ bk, unsigned char* __restrict__ mask) {
  const int lj = -1 + int(blockIdx.x * kIoCols + threadIdx.x);
  const int li = -1 + int(blockIdx.y);
  if (lj > int(G.pitch) - 2 || li > G.nx + 3) return;
  const int gi = G.gi0 + li, gj = G.gj0 + lj;
  const bool node = gi >= 0 && gi <= G.M && gj >= 0 && gj <= G.N;
  double a = 1.0, b = 1.0;
  if (node) {
    auto kv = [&](int i, int j) { return k ? k[int64_t(i) * ld + j] : 1.0; };
    const double kc = kv(gi, gj);
    if (gi >= 1) a = (0.5 * (kv(gi - 1, gj) + kc)) * geo::ls_coef_a(phi, ldp, G.M, G.N, G.eps, gi, gj);
    if (gj >= 1) b = (0.5 * (kv(gi, gj - 1) + kc)) * geo::ls_coef_b(phi, ldp, G.M, G.N, G.eps, gi, gj);
  }
  const int64_t o = int64_t(li) * G.pitch + lj;
  ak[o] = static_cast<T>(a);
  if (li <= G.nx + 2) bk[o] = static_cast<T>(b);
  if (li >= 1 && li <= G.nx && lj >= 1 && lj <= G.ny)  // an owned node: an interior node of the box
    mask[int64_t(li - 1) * G.pitch + lj] = geo::ls_inside(phi, ldp, gi, gj) ? 1 : 0;
}

// local nodes (li0 .. li0 + rows - 1) x (lj0 .. lj0 + cols - 1) of a subdomain whose local (0, 0) is
// global (gi0, gj0); w, pa, pb point to local (0, 0)
template <typename T>
__global__ void __launch_bounds__(kIoCols)
k_gather(const T* __restrict__ w, const T* __restrict__ pa, double ca, const T* __restrict__ pb, double cb,
         int npend, int64_t pitch, double* __restrict__ out, int64_t ld, int li0, int lj0, int rows, int cols,
         int gi0, int gj0, int M, int N) {
  const int c = blockIdx.x * kIoCols + threadIdx.x;
  const int r0 = blockIdx.y * kIoRows;
  if (c >= cols) return;
  const int lj = lj0 + c, gj = gj0 + lj;
  double v[kIoRows];
#pragma unroll
  for (int u = 0; u < kIoRows; ++u) {
    const int li = li0 + r0 + u, gi = gi0 + li;
    v[u] = 0.0;
    if (r0 + u < rows && gi > 0 && gi < M && gj > 0 && gj < N) {
      const int64_t k = int64_t(li) * pitch + lj;
      double x = double(w[k]);
      if (npend > 0) x = __builtin_fma(ca, double(pa[k]), x);
      if (npend > 1) x = __builtin_fma(cb, double(pb[k]), x);
      if (npend > 0 && sizeof(T) == 4) x = double(static_cast<float>(x));
      v[u] = x;
    }
  }
#pragma unroll
  for (int u = 0; u < kIoRows; ++u)
    if (r0 + u < rows) out[int64_t(gi0 + li0 + r0 + u) * ld + gj] = v[u];
}

template <typename T>
void launch_scatter(const double* src, int64_t ld, T* dst, int64_t pitch, int rows, int cols, hipStream_t s) {
  hipLaunchKernelGGL((k_scatter<T>), io_grid(rows, cols), dim3(kIoCols), 0, s, src, ld, dst, pitch, rows, cols);
  HIP_CHECK(hipGetLastError());
}
template void launch_scatter<double>(const double*, int64_t, double*, int64_t, int, int, hipStream_t);
template void launch_scatter<float>(const double*, int64_t, float*, int64_t, int, int, hipStream_t);

template <typename T>
void launch_scatter_shift(const double* src, int64_t ld, T* dst, int64_t pitch, int rows, int cols, double sigma,
                          hipStream_t s) {
  hipLaunchKernelGGL((k_scatter_shift<T>), io_grid(rows, cols), dim3(kIoCols), 0, s, src, ld, dst, pitch, rows, cols,
                     sigma);
  HIP_CHECK(hipGetLastError());
}
template void launch_scatter_shift<double>(const double*, int64_t, double*, int64_t, int, int, double, hipStream_t);
template void launch_scatter_shift<float>(const double*, int64_t, float*, int64_t, int, int, double, hipStream_t);

void launch_value_check(FieldRule rule, const double* field, int64_t ld, int M, int N, int* flag, hipStream_t s) {
  const bool inner = rule == FieldRule::kNonNegInterior;  // the interior nodes only
  const double* src = inner ? field + ld + 1 : field;
  const int rows = inner ? M - 1 : M + 1, cols = inner ? N - 1 : N + 1;
  const auto k = rule == FieldRule::kFinite ? k_finite : inner ? k_reaction_check : k_diffusion_check;
  hipLaunchKernelGGL(k, io_grid(rows, cols), dim3(kIoCols), 0, s, src, ld, rows, cols, flag);
  HIP_CHECK(hipGetLastError());
}

template <typename T>
void launch_face_fields(const DevGeom& G, const DevTables& Tb, const double* k, int64_t ld, T* ak, T* bk, hipStream_t s) {
  PMX_CHECK(k && ak && bk && ld >= G.N + 1, "face fields: need the nodal field (row stride >= N + 1) and both outputs");
  PMX_CHECK(G.nx + 5 <= 65535, "face fields: too many rows for one launch: " << G.nx);
  const dim3 grid(unsigned((G.pitch + kIoCols - 1) / kIoCols), unsigned(G.nx + 5));
  hipLaunchKernelGGL((k_face_fields<T>), grid, dim3(kIoCols), 0, s, G, Tb, k, ld, ak, bk);
  HIP_CHECK(hipGetLastError());
}
template void launch_face_fields<double>(const DevGeom&, const DevTables&, const double*, int64_t, double*, double*,
                                         hipStream_t);
template void launch_face_fields<float>(const DevGeom&, const DevTables&, const double*, int64_t, float*, float*,
                                        hipStream_t);

template <typename T>
void launch_domain_fields(const DevGeom& G, const double* phi, int64_t ldp, const double* k, int64_t ld, T* ak, T* bk,
                          unsigned char* mask, hipStream_t s) {
  PMX_CHECK(phi && ak && bk && mask && ldp >= G.N + 1 && (!k || ld >= G.N + 1),
            "domain fields: need the level-set field (row stride >= N + 1), both outputs and the mask");
  PMX_CHECK(G.nx + 5 <= 65535, "domain fields: too many rows for one launch: " << G.nx);
  const dim3 grid(unsigned((G.pitch + kIoCols - 1) / kIoCols), unsigned(G.nx + 5));
  hipLaunchKernelGGL((k_domain_fields<T>), grid, dim3(kIoCols), 0, s, G, phi, ldp, k, ld, ak, bk, mask);
  HIP_CHECK(hipGetLastError());
}
template void launch_domain_fields<double>(const DevGeom&, const double*, int64_t, const double*, int64_t, double*,
                                           double*, unsigned char*, hipStream_t);
template void launch_domain_fields<float>(const DevGeom&, const double*, int64_t, const double*, int64_t, float*,
                                          float*, unsigned char*, hipStream_t);

template <typename T>
void launch_gather(const T* w, const T* pa, double ca, const T* pb, double cb, int npend, int64_t pitch,
                   double* out, int64_t ld, int li0, int lj0, int rows, int cols, int gi0, int gj0, int M, int N,
                   hipStream_t s) {
  hipLaunchKernelGGL((k_gather<T>), io_grid(rows, cols), dim3(kIoCols), 0, s, w, pa, ca, pb, cb, npend, pitch, out,
                     ld, li0, lj0, rows, cols, gi0, gj0, M, N);
  HIP_CHECK(hipGetLastError());
}
template void launch_gather<double>(const double*, const double*, double, const double*, double, int, int64_t,
                                    double*, int64_t, int, int, int, int, int, int, int, int, hipStream_t);
template void launch_gather<float>(const float*, const float*, double, const float*, double, int, int64_t, double*,
                                   int64_t, int, int, int, int, int, int, int, int, hipStream_t);

}  // namespace pmx
