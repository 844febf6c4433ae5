// CPU PCG — the validation oracle and the "no-GPU" configuration
// (components C4-C10 and P1 of SURVEY §2; stages 0/1/2/3 of the reference).
//
//  * cpu_solve()            : global grid, serial or OpenMP (stage 0 / stage 1 semantics,
//                             stage0/Withoutopenmp1.cpp:106-172, stage1-openmp/Withopenmp1.cpp:133-199)
//  * CpuSubdomain           : one rank's block with a 1-cell halo, phase-structured so the same
//                             code runs under an in-process multi-subdomain driver
//                             (cpu_solve_decomposed) and under MPI (apps/pmx_mpi.cpp)
//                             (stage2-mpi/poisson_mpi_decomp.cpp:356-460, stage3-openmp+mpi/hybrid.cpp:364-470)
#pragma once

#include <cstdint>
#include <functional>
#include <vector>

#include "pmx/decomp.hpp"
#include "pmx/geometry.hpp"
#include "pmx/spec.hpp"

namespace pmx {

struct SolveResult {
  int64_t iters = 0;
  Status status = Status::kRunning;
  double last_diff = 0.0;  // final ||w^{k+1}-w^k|| (norm per spec.norm)
  double seconds = 0.0;    // solver wall time
  // StopRule::kResidual only (0 under the step rule): sqrt(rho) at the end and sqrt(rho_B), see spec.hpp
  double residual = 0.0, residual_ref = 0.0;
  // solution on the global grid, (M+1) x (N+1) row-major, boundary = 0
  std::vector<double> w;
};

// Serial (threads<=1) or OpenMP PCG over the whole grid.
// rhs / w0: optional global (M+1) x (N+1) row-major arrays.  rhs replaces the constant F as
// right-hand side under the ellipse mask (B = rhs inside D, 0 elsewhere; boundary nodes ignored),
// w0 the zero initial iterate (its boundary nodes count as 0): r^0 = B - A w0 in mat_A's arithmetic.
// reaction: optional global field c(x, y) >= 0 next to spec.sigma: the operator is A + (sigma + c) I and the
// Jacobi diagonal D + sigma + c on every interior node (boundary values are not read).  The shift enters
// through the one expression sigma uses, so a constant field equals the sigma solve bitwise.
// diffusion: optional global field k(x, y) of nodal values, finite and > 0 on EVERY node (the faces next to the
// box boundary read its boundary values): the operator is -div(k grad u) + (sigma + c) u, with the face
// coefficients a[i,j] <- (0.5 (k[i-1,j] + k[i,j])) a[i,j], b[i,j] <- (0.5 (k[i,j-1] + k[i,j])) b[i,j] -- the
// fictitious coefficient 1/eps included, so the medium outside D is k/eps -- and everything else the same
// algebra on them.  k = 1 multiplies by exactly 1.0: the solve without the argument, bitwise.
// domain: optional global field phi of nodal level-set values, finite on every node: D = {phi < 0} replaces the
// ellipse.  The face coefficients are geo::ls_coef_a / ls_coef_b of phi (geometry.hpp: cell-centre means, one
// linear crossing per face, theta + (1 - theta) / eps) and the right-hand-side mask is phi < 0 on the node;
// diffusion scales those faces as it scales the ellipse's.
SolveResult cpu_solve(const ProblemSpec& spec, int threads = 1, bool keep_solution = true,
                      const double* rhs = nullptr, const double* w0 = nullptr, const double* reaction = nullptr,
                      const double* diffusion = nullptr, const double* domain = nullptr);

// Assemble the reference's 2D arrays on the host (tests: kernel bit-equality).
// a, b are (M+2) x (N+2) including ghost nodes; B is (M+1) x (N+1).  domain: as cpu_solve.
void cpu_assemble(const ProblemSpec& spec, std::vector<double>& a, std::vector<double>& b,
                  std::vector<double>& B, const double* domain = nullptr);

// The operator itself, the host twin of Session::apply_device: alpha L x + beta x + gamma y + c0 on the interior
// nodes and 0 on the box boundary of a global (M+1) x (N+1) row-major array, L = A + spec.sigma I -- the plain
// matrix on the whole box, no ellipse mask -- in cpu_solve's mat_A arithmetic.  Boundary values of x count as 0
// and are not read; y may be null (no y term).  Combination order: v = alpha Lx; v = fma(beta, x, v);
// v = fma(gamma, y, v) with y; v += c0 -- and Lx itself for alpha = 1, beta = 0, no y, c0 = 0.
// reaction, diffusion, domain: as cpu_solve (L = A_k + (sigma + c) I, A_k on the faces of the domain).
std::vector<double> cpu_apply(const ProblemSpec& spec, const double* x, const double* y = nullptr, double alpha = 1.0,
                              double beta = 0.0, double gamma = 1.0, double c0 = 0.0, const double* reaction = nullptr,
                              const double* diffusion = nullptr, const double* domain = nullptr);

// One rank's block (local arrays (nx+2) x (ny+2), row-major, pitch ny+2).
class CpuSubdomain {
 public:
  // rhs / w0 / reaction / diffusion / domain: as cpu_solve (global arrays; this block, and for w0 its ring, are
  // copied; domain and diffusion are folded into the block's face coefficients and mask)
  CpuSubdomain(const ProblemSpec& spec, const Subdomain& sd, int threads, const double* rhs = nullptr,
               const double* w0 = nullptr, const double* reaction = nullptr, const double* diffusion = nullptr,
               const double* domain = nullptr);

  const Subdomain& sd() const { return sd_; }
  int pitch() const { return sd_.ny + 2; }

  double init();                         // r=B-A w0, z=D^-1 r, p=z, w=w0 (0) -> local (z,r)
  double matvec_dot();                   // Ap = A p (needs p halos) -> local (Ap,p)
  void update_wr(double alpha, double* diff_local);   // w+=ap, r-=aAp, local sum dw^2
  double precond_dot();                  // z = D^-1 r -> local (z,r)
  double rhs_dot() const;                // local (D^-1 B, B): the residual rule's reference (spec.hpp)
  bool has_w0() const { return !w0_.empty(); }
  void update_p(double beta);            // p = z + beta p

  // halo access for p (the only field with halos, stage2-mpi/poisson_mpi_decomp.cpp:241-347)
  // side: 0 = x-lo (row 1), 1 = x-hi (row nx), 2 = y-lo (col 1), 3 = y-hi (col ny)
  int edge_len(int side) const { return side < 2 ? sd_.ny : sd_.nx; }
  void get_edge(int side, double* out) const;
  void set_ghost(int side, const double* in);
  void zero_ghost(int side);

  // gather local interior of w into a global (M+1)x(N+1) array
  void scatter_w_into(std::vector<double>& global) const;

 private:
  ProblemSpec spec_;
  GridInfo g_;
  Subdomain sd_;
  int threads_;
  std::vector<double> a_, b_, B_, w_, r_, z_, p_, Ap_;
  std::vector<double> w0_;  // initial iterate with its ring (empty: zero)
  std::vector<double> sh_;  // sigma + c on the owned nodes (empty: no reaction field, the shift is spec.sigma)
};

// In-process multi-subdomain driver: P subdomains stepped in lock-step with a
// deterministic rank-ordered reduction.  This is the "fake cluster" used to test
// decomposition + halo logic without MPI (SURVEY §4.2 'distributed (fake)').
SolveResult cpu_solve_decomposed(const ProblemSpec& spec, int nranks, Split split,
                                 int threads_per_rank = 1, bool keep_solution = true,
                                 const double* rhs = nullptr, const double* w0 = nullptr,
                                 const double* reaction = nullptr, const double* diffusion = nullptr,
                                 const double* domain = nullptr);

// Generic lock-step PCG over CpuSubdomains with pluggable collectives.  The MPI
// app supplies MPI-backed callbacks; the in-process driver supplies local ones.
struct HostCollectives {
  std::function<double(double)> allreduce_sum;          // global sum of one double
  std::function<void(CpuSubdomain&)> exchange_p_halos;  // fill p ghosts (Dirichlet zero at boundary)
};
SolveResult cpu_pcg_loop(const ProblemSpec& spec, std::vector<CpuSubdomain*>& local,
                         HostCollectives& coll);

}  // namespace pmx
