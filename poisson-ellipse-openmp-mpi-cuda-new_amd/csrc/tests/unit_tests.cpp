// Native unit tests of the host core (SURVEY §4.2 "unit (CPU)"): geometry, decomposition, CPU
// PCG goldens, report formats.  No framework: each CHECK prints file:line on failure and the
// binary exits non-zero.  Built as bin/pmx_unit_tests by utils/build.py and as a CTest target by
// CMakeLists.txt; tests/test_native_unit.py runs it under pytest.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <sstream>
#include <string>
#include <vector>

#include "pmx/cpu_pcg.hpp"
#include "pmx/decomp.hpp"
#include "pmx/geometry.hpp"
#include "pmx/memory_plan.hpp"
#include "pmx/operator.hpp"
#include "pmx/report.hpp"
#include "pmx/spec.hpp"

namespace {

int g_failed = 0, g_checks = 0;

#define CHECK(cond)                                                         \
  do {                                                                      \
    ++g_checks;                                                             \
    if (!(cond)) {                                                          \
      ++g_failed;                                                           \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
    }                                                                       \
  } while (0)

using namespace pmx;

// stage2-mpi/poisson_mpi_decomp.cpp:60-64: Px = floor(sqrt(P)), decremented until it divides P
void test_process_grid() {
  const int expect[][3] = {{1, 1, 1}, {2, 1, 2}, {3, 1, 3}, {4, 2, 2}, {6, 2, 3},
                           {7, 1, 7}, {8, 2, 4}, {12, 3, 4}, {16, 4, 4}, {20, 4, 5}};
  for (const auto& e : expect) {
    const ProcGrid g = choose_process_grid(e[0]);
    CHECK(g.Px == e[1] && g.Py == e[2]);
  }
  CHECK(make_process_grid(8, 16384, 16384, Split::kRows).Px == 8);
  CHECK(make_process_grid(8, 16384, 16384, Split::kCols).Py == 8);
}

// every interior node owned exactly once; sizes differ by <= 1; neighbours are symmetric
void test_decomposition_cover() {
  for (int P : {1, 2, 3, 4, 6, 7, 8, 12}) {
    const int M = 97, N = 131;
    const ProcGrid g = choose_process_grid(P);
    std::vector<int> owner(size_t(M + 1) * (N + 1), -1);
    int nx_min = 1 << 30, nx_max = 0, ny_min = 1 << 30, ny_max = 0;
    for (int r = 0; r < P; ++r) {
      const Subdomain d = decompose_2d(M, N, g, r);
      nx_min = std::min(nx_min, d.nx); nx_max = std::max(nx_max, d.nx);
      ny_min = std::min(ny_min, d.ny); ny_max = std::max(ny_max, d.ny);
      for (int i = d.i_start; i <= d.i_end; ++i)
        for (int j = d.j_start; j <= d.j_end; ++j) {
          int& o = owner[size_t(i) * (N + 1) + j];
          CHECK(o == -1);
          o = r;
        }
      const int nbs[4] = {d.nb_xlo, d.nb_xhi, d.nb_ylo, d.nb_yhi};
      for (int s = 0; s < 4; ++s) {
        if (nbs[s] < 0) continue;
        const Subdomain n = decompose_2d(M, N, g, nbs[s]);
        const int back[4] = {n.nb_xlo, n.nb_xhi, n.nb_ylo, n.nb_yhi};
        CHECK(back[s ^ 1] == r);
      }
    }
    for (int i = 1; i < M; ++i)
      for (int j = 1; j < N; ++j) CHECK(owner[size_t(i) * (N + 1) + j] >= 0);
    CHECK(nx_max - nx_min <= 1 && ny_max - ny_min <= 1);
  }
}

// coefficient invariants: 1 deep inside D, 1/eps far outside, symmetric about both axes
void test_geometry() {
  ProblemSpec s;
  s.M = 80; s.N = 60;
  const GridInfo g(s);
  const geo::FaceTables t(s, g);
  CHECK(geo::inside(0.0, 0.0, s.ax, s.by, true));
  CHECK(!geo::inside(0.99, 0.45, s.ax, s.by, true));
  CHECK(geo::coef_a(t, g, s.M / 2, s.N / 2) == 1.0);
  CHECK(geo::coef_b(t, g, s.M / 2, s.N / 2) == 1.0);
  CHECK(geo::coef_a(t, g, 1, 1) == g.inv_eps);
  for (int i = 1; i <= s.M; ++i)
    for (int j = 1; j <= s.N; ++j) {
      // a(i, j) uses the face at x_i - h1/2: mirror i -> M + 1 - i, j -> N - j
      const double a = geo::coef_a(t, g, i, j), am = geo::coef_a(t, g, s.M + 1 - i, s.N - j);
      CHECK(std::fabs(a - am) <= 1e-9 * std::fabs(a));
    }
  // analytic solution vanishes on the ellipse, F / (2/ax^2 + 2/by^2) at the centre
  CHECK(std::fabs(geo::exact_solution(0.0, 0.0, s) - 0.1) < 1e-15);
  CHECK(geo::exact_solution(1.0, 0.0, s) == 0.0);
}

// SURVEY §4.1 goldens (reproduced from the reference code)
void test_cpu_goldens() {
  const int weighted[][3] = {{10, 10, 15}, {20, 20, 26}, {40, 40, 50}};
  for (const auto& e : weighted) {
    ProblemSpec s;
    s.M = e[0]; s.N = e[1];
    const SolveResult r = cpu_solve(s, 1, true);
    CHECK(r.status == Status::kConverged && r.iters == e[2]);
  }
  const int unweighted[][3] = {{10, 10, 17}, {20, 20, 31}, {40, 40, 61}};
  for (const auto& e : unweighted) {
    ProblemSpec s;
    s.M = e[0]; s.N = e[1]; s.norm = Norm::kUnweighted;
    CHECK(cpu_solve(s, 1, false).iters == e[2]);
  }
  ProblemSpec s;  // 40x40: max w and error vs analytic
  const SolveResult r = cpu_solve(s, 1, true);
  const ErrorNorms e = error_norms(s, r.w);
  CHECK(std::fabs(e.max_w - 0.09797040155) < 1e-9);
  CHECK(std::fabs(e.l2 - 3.6773e-3) < 1e-7);
  // threaded decomposition reproduces the serial solve
  const SolveResult d = cpu_solve_decomposed(s, 4, Split::kReference, 1, true);
  CHECK(d.iters == r.iters);
  double dmax = 0.0;
  for (size_t k = 0; k < r.w.size(); ++k) dmax = std::max(dmax, std::fabs(d.w[k] - r.w[k]));
  CHECK(dmax < 1e-12);
}

void test_report_formats() {
  JsonLine j;
  j.ks("backend", "cpu").kv("M", 40).kv("x", 0.125);
  CHECK(j.str() == "{\"backend\": \"cpu\", \"M\": 40, \"x\": 0.125}");
  CHECK(std::string(status_name(Status::kConverged)) == "converged");
  CHECK(std::string(status_name(Status::kBreakdown)) == "breakdown");
}

void test_spec_validation() {
  ProblemSpec s;
  s.M = 1;
  bool threw = false;
  try { s.validate(); } catch (const Error&) { threw = true; }
  CHECK(threw);
  ProblemSpec t;
  CHECK(t.effective_max_iter() == 39 * 39);
  t.max_iter = 7;
  CHECK(t.effective_max_iter() == 7);
}

// MemoryPlan: the conditions the solver's kernels rely on, for every algorithm, storage type and ghost-row
// count, on one grid, 2 x 2 blocks and row strips
void test_memory_plan() {
  const int grids[][2] = {{40, 40}, {97, 130}, {16384, 16384}};
  const struct { int world; Split split; } decomps[] = {{1, Split::kAuto}, {4, Split::kReference}, {8, Split::kRows}};
  for (const auto& mn : grids)
    for (const auto& dc : decomps)
      for (int rank : {0, dc.world - 1})
        for (DType dtype : {DType::kFp64, DType::kFp32})
          for (int algo : {1, 2, 3})
            for (int gh : {2, 3, 6}) {
              ProblemSpec spec;
              spec.M = mn[0];
              spec.N = mn[1];
              const Subdomain sd = decompose_2d(spec.M, spec.N, make_process_grid(dc.world, spec.M, spec.N, dc.split), rank);
              const MemoryPlan p(spec, sd, dtype, algo, gh);
              const bool blocks = algo == 3 && sd.grid.Py > 1;  // s-step 2-D blocks: gh ghost columns per side
              const int64_t cols = blocks ? gh : 1;             // ghost columns on each side
              CHECK(p.elem == (dtype == DType::kFp64 ? 8u : 4u) && p.align * p.elem == 256 && p.gh == gh);
              CHECK(p.nfields == (algo == 2 ? 4 : 5) && (p.face_bytes != 0) == (algo == 3));
              // column 1 of every row of every field (and face field) starts a 256-B line of the allocation
              bool aligned = true;
              for (int f = 0; f < p.nfields; ++f)
                for (int64_t li = 1 - gh; li <= sd.nx + gh; ++li) aligned = aligned && p.at(f, li, 1) % 256 == 0;
              for (int f = 0; f < 2 && algo == 3; ++f)
                for (int64_t li = 1 - gh; li <= sd.nx + gh; ++li) aligned = aligned && p.face_at(f, li, 1) % 256 == 0;
              CHECK(aligned);
              // a field holds its first ghost row from its leftmost column to its last row's rightmost one
              CHECK(int64_t(p.field_off) + (1 - gh) * p.pitch - (cols - 1) >= 0);
              CHECK(p.at(0, sd.nx + gh, sd.ny + cols) + p.elem <= p.field_bytes);
              CHECK(p.at(1, 1 - gh, 1 - cols) >= p.field_bytes);  // ... and the next field starts behind it
              if (algo == 3) CHECK(p.face_at(0, sd.nx + gh, sd.ny + cols) + 8 <= p.face_bytes);
              // 2-D blocks: a row's right ghost columns end before the next row's left ones begin
              if (blocks) CHECK(p.at(0, 0, sd.ny + gh) < p.at(0, 1, -gh));
              CHECK(p.row_bytes() == size_t(p.pitch) * p.elem && p.pitch >= sd.ny + 2 + 8);
              const size_t tables = (4 * size_t(spec.M + 2) + 4 * size_t(spec.N + 2)) * 8 + 8 * size_t(spec.M + 2) * 4;
              CHECK(p.table_bytes == tables);
              CHECK(p.total() == size_t(p.nfields) * p.field_bytes + 2 * p.face_bytes + tables);
            }
}

// the operator members of InitData<double> and ApplyCoef (HIP headers), as set_operator fills them
struct InitData4 {
  double sigma = 0.0;
  const double *shift = nullptr, *ka = nullptr, *kb = nullptr;
};

// OperatorData::kind(): the one rule that picks the kernels, and k_pcg1's (SH, DIF) pair
void test_operator_kind() {
  const double f[3] = {0.0, 0.0, 0.0};
  using Op = OperatorData<double>;
  CHECK((Op{}.kind() == OpKind::kPlain));
  CHECK((Op{2.5, nullptr, nullptr, nullptr}.kind() == OpKind::kSigma));
  CHECK((Op{0.0, f, nullptr, nullptr}.kind() == OpKind::kField));
  CHECK((Op{2.5, f, nullptr, nullptr}.kind() == OpKind::kField));
  CHECK((Op{0.0, f, f + 1, f + 2}.kind() == OpKind::kDiffusion));
  CHECK((Op{2.5, f, f + 1, f + 2}.kind() == OpKind::kDiffusion));
  CHECK((OperatorData<void>{0.0, f, f, f}.kind() == OpKind::kDiffusion));  // type-erased, as ApplyCoef
  for (const Op& bad : {Op{0.0, nullptr, f, f}, Op{0.0, f, f, nullptr}, Op{1.0, nullptr, f, nullptr}}) {
    bool threw = false;
    try { (void)bad.kind(); } catch (const Error&) { threw = true; }
    CHECK(threw);
  }
  // the enum's values are the SH of k_init and k_apply; k_pcg1 takes SH = min(kind, 2) and DIF = (kind == 3)
  CHECK(int(OpKind::kPlain) == 0 && int(OpKind::kSigma) == 1 && int(OpKind::kField) == 2 && int(OpKind::kDiffusion) == 3);
  const struct { OpKind k; int sh; bool dif; } map[] = {{OpKind::kPlain, 0, false}, {OpKind::kSigma, 1, false},
                                                        {OpKind::kField, 2, false}, {OpKind::kDiffusion, 2, true}};
  for (const auto& m : map) {
    CHECK(pcg1_sh(m.k) == m.sh && pcg1_dif(m.k) == m.dif);
    CHECK(with_op_kind(m.k, [](auto K) { return decltype(K)::value; }) == m.k);
  }
  InitData4 x;
  set_operator(x, Op{2.5, f, f + 1, f + 2});
  CHECK(x.sigma == 2.5 && x.shift == f && x.ka == f + 1 && x.kb == f + 2);
}

// field_values_ok on 5 x 6 nodes (M = 4, N = 5) with row stride 8: the padding holds NaN and is never read
void test_field_values() {
  const int M = 4, N = 5, ld = 8;
  const double inf = HUGE_VAL, nan = std::nan("");
  std::vector<double> clean(size_t(M + 1) * ld, nan);
  for (int i = 0; i <= M; ++i)
    for (int j = 0; j <= N; ++j) clean[size_t(i) * ld + j] = 1.0 + 0.25 * i + 0.125 * j;
  const FieldRule rules[3] = {FieldRule::kFinite, FieldRule::kNonNegInterior, FieldRule::kPositive};
  for (FieldRule r : rules) CHECK(field_values_ok(clean.data(), ld, M, N, r));
  // value -> passes {kFinite, kNonNegInterior, kPositive} where the rule reads the node
  const struct { double v; bool ok[3]; } vals[] = {{nan, {false, false, false}}, {inf, {false, false, false}},
                                                   {-1.0, {true, false, false}}, {0.0, {true, true, false}},
                                                   {-0.0, {true, true, false}}};
  const int interior[][2] = {{1, 1}, {2, 3}, {M - 1, N - 1}};
  const int boundary[][2] = {{0, 0}, {0, 2}, {2, 0}, {M, 3}, {1, N}, {M, N}};
  for (const auto& t : vals) {
    for (const auto& n : interior) {
      std::vector<double> a = clean;
      a[size_t(n[0]) * ld + n[1]] = t.v;
      for (int r = 0; r < 3; ++r) CHECK(field_values_ok(a.data(), ld, M, N, rules[r]) == t.ok[r]);
    }
    for (const auto& n : boundary) {  // kNonNegInterior never reads the box boundary
      std::vector<double> a = clean;
      a[size_t(n[0]) * ld + n[1]] = t.v;
      CHECK(field_values_ok(a.data(), ld, M, N, FieldRule::kFinite) == t.ok[0]);
      CHECK(field_values_ok(a.data(), ld, M, N, FieldRule::kNonNegInterior));
      CHECK(field_values_ok(a.data(), ld, M, N, FieldRule::kPositive) == t.ok[2]);
    }
  }
  CHECK(field_values_ok(clean.data(), ld, M, N, FieldRule::kFinite));  // (the copies were the ones changed)
  CHECK(std::string("rhs") + field_rule_text(FieldRule::kFinite) == "rhs holds non-finite values");
  CHECK(std::string("reaction") + field_rule_text(FieldRule::kNonNegInterior) ==
        "reaction must be finite and >= 0 on every interior node");
  CHECK(std::string("diffusion") + field_rule_text(FieldRule::kPositive) ==
        "diffusion must be finite and > 0 on every node");
}

}  // namespace

int main() {
  test_process_grid();
  test_decomposition_cover();
  test_geometry();
  test_cpu_goldens();
  test_report_formats();
  test_spec_validation();
  test_memory_plan();
  test_operator_kind();
  test_field_values();
  std::printf("pmx_unit_tests: %d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
