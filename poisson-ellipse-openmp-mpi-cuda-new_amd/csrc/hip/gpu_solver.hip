// GPU PCG subdomain solver (GpuSubdomainSolver: fields, tables, placement probe, kernels, checkpoints).
// See pmx/gpu_solver.hpp.  The iteration driver (PcgDriver: streams, graphs, batches, phase buckets)
// is in pcg_driver.hip; the s-step solver's passes and its driver schedule in ca_solver.hip, pcg1's
// decomposed-grid schedules in pcg1_driver.hip.
//
// Reference call stack being replaced (stage4-mpi+cuda/poisson_mpi_cuda_f.cu:688-983): CPU
// assembly + 3 H2D copies, 8 cudaMallocs, and per iteration 8 launches each followed by
// cudaDeviceSynchronize, 3x256-KiB partial D2H copies with host summation, host-staged halos.
// Here per iteration: 4 launches (2 streaming + 2 single-block reductions), zero host syncs,
// replayed from a hipGraph in batches.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <sstream>
#include <stdexcept>
#include <unistd.h>
#include <string>
#include <vector>
#include <istream>
#include <ostream>

#include "pmx/common.hpp"
#include "pmx/gpu_solver.hpp"
#include "pmx/session.hpp"
#include "pmx/trace.hpp"

namespace pmx {

namespace {
size_t round_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
double now_s() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
template <typename T> DevPtr<T> dev_alloc(size_t bytes) {
  T* p = nullptr;
  HIP_CHECK(hipMalloc(&p, bytes));
  return DevPtr<T>(p);
}
Stream make_stream() {
  hipStream_t s = nullptr;
  HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  return Stream(s);
}
template <typename T> HostPtr<T> host_alloc(size_t bytes, unsigned flags) {
  T* p = nullptr;
  HIP_CHECK(hipHostMalloc(&p, bytes, flags));
  return HostPtr<T>(p);
}
Event make_event(unsigned flags = hipEventDefault) {
  hipEvent_t e = nullptr;
  HIP_CHECK(hipEventCreateWithFlags(&e, flags));
  return Event(e);
}
}  // namespace

DevGeom make_dev_geom(const ProblemSpec& spec, const Subdomain& sd, int64_t pitch) {
  const GridInfo g(spec);
  DevGeom G{};
  G.nx = sd.nx;
  G.ny = sd.ny;
  G.pitch = pitch;
  G.gi0 = sd.gi0();
  G.gj0 = sd.gj0();
  G.M = spec.M;
  G.N = spec.N;
  G.nb = 0;  // slot s <-> bit 1 << s (kNbXlo .. kNbXhiYhi)
  for (int s = 0; s < kHaloSlots; ++s) G.nb |= sd.peer(s) >= 0 ? 1 << s : 0;
  G.ref_ellipse = spec.reference_ellipse() ? 1 : 0;
  G.h1 = g.h1; G.h2 = g.h2; G.eps = g.eps; G.inv_eps = g.inv_eps; G.h1h2 = g.h1h2;
  G.cx = 1.0 / (g.h1 * g.h1);
  G.cy = 1.0 / (g.h2 * g.h2);
  // D + sigma of the uniform stencils (sigma = 0: D + 0.0 is D, bit for bit)
  G.dinv_in = 1.0 / (((1.0 + 1.0) * G.cx + (1.0 + 1.0) * G.cy) + spec.sigma);
  G.dinv_out = 1.0 / (((g.inv_eps + g.inv_eps) * G.cx + (g.inv_eps + g.inv_eps) * G.cy) + spec.sigma);
  G.ax = spec.ax; G.by = spec.by; G.F = spec.F;
  return G;
}

DevTables upload_tables(const ProblemSpec& spec, double** owner) {
  const GridInfo g(spec);
  const geo::FaceTables ft(spec, g);
  const size_t nxT = spec.M + 2, nyT = spec.N + 2;
  const size_t ndbl = 4 * nxT + 4 * nyT, nint = 8 * nxT;
  DevPtr<double> buf = dev_alloc<double>(ndbl * sizeof(double) + nint * sizeof(int));
  std::vector<double> host(ndbl);
  double* h = host.data();
  std::memcpy(h + 0 * nxT, ft.rv.data(), nxT * 8);
  std::memcpy(h + 1 * nxT, ft.xlo.data(), nxT * 8);
  std::memcpy(h + 2 * nxT, ft.xhi.data(), nxT * 8);
  std::memcpy(h + 3 * nxT, ft.x.data(), nxT * 8);
  double* hy = h + 4 * nxT;
  std::memcpy(hy + 0 * nyT, ft.rh.data(), nyT * 8);
  std::memcpy(hy + 1 * nyT, ft.ylo.data(), nyT * 8);
  std::memcpy(hy + 2 * nyT, ft.yhi.data(), nyT * 8);
  std::memcpy(hy + 3 * nyT, ft.y.data(), nyT * 8);
  HIP_CHECK(hipMemcpy(buf.get(), host.data(), ndbl * 8, hipMemcpyHostToDevice));
  const double* d = buf.get();
  const double* dy = d + 4 * nxT;
  int* cls = reinterpret_cast<int*>(buf.get() + ndbl);
  DevTables T{d, d + nxT, d + 2 * nxT, d + 3 * nxT, dy, dy + nyT, dy + 2 * nyT, dy + 3 * nyT,
              cls, cls + 4 * nxT};
  // classify every row on the device with the exact coefficient formulas
  Subdomain whole;
  whole.M = spec.M; whole.N = spec.N; whole.nx = spec.M - 1; whole.ny = spec.N - 1;
  launch_classify(make_dev_geom(spec, whole, spec.N + 2), T, cls, cls + 4 * nxT, nullptr);
  HIP_CHECK(hipDeviceSynchronize());
  *owner = buf.release();
  return T;
}

namespace {
bool study_mode() {
  const char* e = std::getenv("PMX_STUDY");
  return e && e[0] == '1';
}
// one warning per process for knob variables that are set outside study mode
void warn_ignored_knobs() {
  static std::once_flag once;
  std::call_once(once, [] {
    std::string names;
    for (char** e = ::environ; e && *e; ++e) {
      const std::string kv = *e;
      const std::string k = kv.substr(0, kv.find('='));
      static const char* knobs[] = {"PMX_ALGO", "PMX_PAIR_W", "PMX_PCG1_", "PMX_CA_", "PMX_ARITH32", "PMX_PLACEMENT",
                                    "PMX_DIRECT_ROWS", "PMX_FRAME_ON_COMM", "PMX_FORK_ONE_QUEUE", "PMX_LOOPBACK_",
                                    "PMX_IPC_COARSE", "PMX_PROGRESS"};
      for (const char* p : knobs)
        if (k.rfind(p, 0) == 0) names += (names.empty() ? "" : ", ") + k;
    }
    if (!names.empty())
      std::fprintf(stderr, "pmx: ignoring %s (kernel / schedule study knobs apply only with PMX_STUDY=1)\n",
                   names.c_str());
  });
}
}  // namespace

const char* study_env(const char* name) {
  if (!study_mode()) {
    warn_ignored_knobs();
    return nullptr;
  }
  return std::getenv(name);
}

GpuOptions resolve_options(const GpuOptions& in) {
  if (in.resolved) return in;
  GpuOptions o = in;
  const bool study = study_mode();
  if (!study) warn_ignored_knobs();
  auto env_int = [study](const char* name, int& v) {
    if (!study) return;
    if (const char* e = std::getenv(name); e && e[0]) v = std::atoi(e);
  };
  env_int("PMX_PAIR_W", o.pair_w);
  env_int("PMX_ALGO", o.algo);
  env_int("PMX_PCG1_VEC", o.vec1);
  env_int("PMX_PCG1_ROWS", o.rows1);
  env_int("PMX_PCG1_ROWS_W", o.rows1w);
  env_int("PMX_PCG1_PF_W", o.pf1w);
  env_int("PMX_PCG1_WAVES", o.waves1);
  env_int("PMX_PCG1_WAVES_W", o.waves1w);
  env_int("PMX_PCG1_PF", o.pf1);
  env_int("PMX_PCG1_ORDER", o.order1);
  env_int("PMX_PCG1_WCYCLE", o.wcycle1);
  env_int("PMX_PROGRESS", o.progress);
  env_int("PMX_ARITH32", o.arith32);
  env_int("PMX_PLACEMENT", o.placement);
  env_int("PMX_PCG1_WPCU", o.wpcu1);
  env_int("PMX_PCG1_WPCU_W", o.wpcu1w);
  env_int("PMX_PCG1_BLOCK", o.block1);
  env_int("PMX_PCG1_BLOCK_ROWS", o.block_rows1);
  env_int("PMX_PCG1_BLOCK_WAVES", o.block_waves1);
  env_int("PMX_PCG1_BLOCK_FUSED", o.block_fused1);
  PMX_CHECK(o.block1 >= -1 && o.block1 <= 1, "block tiles must be -1 (auto), 0 or 1");
  PMX_CHECK(o.block_rows1 == 0 || pcg1_block_shape_ok(o.block_rows1, o.block_waves1),
            "block tiles: no " << o.block_rows1 << "-row x " << o.block_waves1 << "-wave variant (4/8/12/16 x 8, 8/16 x 16)");
  PMX_CHECK(o.block_waves1 == 8 || o.block_waves1 == 16, "block tiles: 8 or 16 waves per workgroup");
  PMX_CHECK(o.block_fused1 >= -1 && o.block_fused1 <= 1, "block-tile fused reduction must be -1 (auto), 0 or 1");
  env_int("PMX_CA_S", o.ca_s);
  env_int("PMX_CA_ROWS", o.ca_rows);
  env_int("PMX_CA_ROWS_UPD", o.ca_rows2);
  PMX_CHECK(o.ca_s == 2 || o.ca_s == 3, "s-step PCG: s must be 2 or 3");
  PMX_CHECK(o.ca_rows >= 0 && o.ca_rows <= 4096, "s-step PCG: tile rows must be 0 (auto) .. 4096");
  env_int("PMX_CA_DMA", o.ca_dma);
  env_int("PMX_CA_SPLIT", o.ca_split);
  env_int("PMX_CA_FRAME_STREAM", o.ca_frame_stream);
  env_int("PMX_CA_FUSE", o.ca_fuse);
  env_int("PMX_CA_ROWS_F", o.ca_rows_f);
  PMX_CHECK(o.ca_fuse >= -1 && o.ca_fuse <= 1, "s-step PCG: ca_fuse must be -1, 0 or 1");
  PMX_CHECK(o.ca_rows_f >= 0 && o.ca_rows_f <= 4096, "s-step PCG: fused tile rows must be 0 (auto) .. 4096");
  env_int("PMX_CA_DIRICHLET", o.ca_dirichlet);
  if (const char* pk = study ? std::getenv("PMX_PLACEMENT_PICK") : nullptr; pk && pk[0])
    o.placement_pick = std::string(pk) == "slowest" ? 1 : 0;
  env_int("PMX_PCG1_SPLIT", o.split_sweep);
  PMX_CHECK(o.split_sweep >= -1 && o.split_sweep <= 1, "split_sweep must be -1, 0 or 1");
  PMX_CHECK(o.ca_split >= -1 && o.ca_split <= 1, "s-step PCG: ca_split must be -1, 0 or 1");
  PMX_CHECK(o.ca_dma >= -1 && o.ca_dma <= 1, "s-step PCG: ca_dma must be -1, 0 or 1");
  env_int("PMX_PCG1_DMA", o.dma1);
  env_int("PMX_PCG1_DMA_W", o.dma1w);
  PMX_CHECK(o.dma1 == 0 || o.dma1 == 2 || o.dma1 == 3, "pcg1 LDS-DMA prefetch depth must be 0, 2 or 3");
  PMX_CHECK(o.dma1w == -1 || o.dma1w == 0 || o.dma1w == 2 || o.dma1w == 3,
            "pcg1 w-sweep LDS-DMA prefetch depth must be -1, 0, 2 or 3");
  PMX_CHECK(o.wpcu1 >= 0 && o.wpcu1 <= 32 && o.wpcu1w >= 0 && o.wpcu1w <= 32, "pcg1 waves per CU must be 0..32");
  PMX_CHECK(o.wcycle1 == 2 || o.wcycle1 == 3, "pcg1 w cycle must be 2 or 3");
  PMX_CHECK(o.pair_w >= 0 && o.pair_w <= 2, "pair_w must be 0, 1 or 2");
  PMX_CHECK(o.algo >= -1 && o.algo <= 3 && o.algo != 0, "algo must be -1, 1, 2 or 3");
  o.resolved = true;
  return o;
}

void apply_sigma_rules(const ProblemSpec& spec, const ProcGrid& grid, GpuOptions& o) {
  PMX_CHECK(o.resolved, "apply_sigma_rules needs resolve_options()");
  if (spec.sigma == 0.0 && !o.shift_field) return;
  auto refuse = [&](const char* option) {
    throw std::invalid_argument(std::string(o.domain        ? "a level-set domain"
                                            : o.diffusion   ? "a diffusion field"
                                            : o.shift_field ? "a reaction field"
                                                            : "sigma != 0 (the screened problem)") +
                                " runs pcg1 on the row march only: " + option + " is not built for it");
  };
  if (o.algo == 3) refuse("algo=\"ca\" (the s-step PCG)");
  if (o.algo == 2) refuse("algo=\"pcg2\"");
  if (o.exact) refuse("exact=True (the reference's operation order)");
  if (o.block1 == 1) refuse("block_tiles=1");
  if (grid.size() > 1 && ((spec.M - 1) / grid.Px < 2 || (spec.N - 1) / grid.Py < 2))
    refuse("a decomposition into subdomains thinner than 2 nodes");
  o.algo = 1;
  o.block1 = 0;
}

bool choose_single_pass(const ProblemSpec& spec, const ProcGrid& grid, const GpuOptions& o,
                        double device_total_bytes, int subdomains_per_device) {
  PMX_CHECK(o.resolved, "choose_single_pass needs resolve_options()");
  if (o.algo == 2 || o.algo == 3) return false;
  // the radius-2 halo takes two owned lines from every neighbour: each block needs >= 2 x 2
  const bool thick = grid.size() == 1 || ((spec.M - 1) / grid.Px >= 2 && (spec.N - 1) / grid.Py >= 2);
  const bool ok = !o.exact && thick;
  PMX_CHECK(o.algo != 1 || ok, "pcg1 needs the fast arithmetic and subdomains of at least 2 x 2 nodes");
  if (o.algo == 1) return true;
  // auto: every storage type.  (Round 1 kept pcg2 for fp32 -- 32768^2: pcg1 8.99 ms vs pcg2 7.69 --
  // but with the scalar-cache row tables and short tiles pcg1 wins there too: 5.20 vs 7.08 ms,
  // 16384^2 1.41 vs 2.00 ms, profiles/r2/fp32_pcg1_sweep.txt)
  if (!ok) return false;
  if (device_total_bytes > 0) {  // the 5th field must fit (rank 0 holds the largest block)
    const Subdomain sd0 = decompose_2d(spec.M, spec.N, grid, 0);
    const double need = double(GpuSubdomainSolver::estimate_device_bytes_algo(spec, sd0, o.dtype, 1)) *
                        std::max(1, subdomains_per_device);
    if (need > 0.95 * device_total_bytes) return false;
  }
  return true;
}

int choose_algo(const ProblemSpec& spec, const ProcGrid& grid, const GpuOptions& o, double device_total_bytes,
                int subdomains_per_device, bool direct_rows) {
  PMX_CHECK(o.resolved, "choose_algo needs resolve_options()");
  if (o.algo == 3) return 3;  // validated by the solver
  if (o.algo == -1) {
    // one grid, or (native transports) row strips of >= 8 rows / 2-D blocks of >= 8 x 8 nodes (BASELINE
    // config 4: packed ghost rows, columns and corners once per block of s iterations)
    const bool strips = grid.size() == 1 || (direct_rows && (spec.M - 1) / grid.Px >= 8 &&
                                             (grid.Py == 1 || (spec.N - 1) / grid.Py >= 8));
    // every storage type: with fp32 / mixed fields the s-step keeps its basis and sums in fp64 registers
    // and beats pcg1 too (16384^2 0.951 vs 1.093 ms, 32768^2 3.356 vs 3.831; NOTES #124)
    bool ca = !o.exact && strips && int64_t(spec.M - 1) * (spec.N - 1) >= kCaAutoPoints;
    if (ca && device_total_bytes > 0) {  // rank 0 holds the largest strip
      const Subdomain sd0 = decompose_2d(spec.M, spec.N, grid, 0);
      const double need = double(GpuSubdomainSolver::estimate_device_bytes_algo(spec, sd0, o.dtype, 3)) *
                          std::max(1, subdomains_per_device);
      ca = need <= 0.95 * device_total_bytes;
    }
    if (ca) return 3;
  }
  return choose_single_pass(spec, grid, o, device_total_bytes, subdomains_per_device) ? 1 : 2;
}

CommLayout GpuSubdomainSolver::comm_layout(const Subdomain& sd, DType dtype, bool single_pass, int ca_gh) {
  CommLayout L;
  L.elem = dtype == DType::kFp64 ? 8 : 4;
  L.single_pass = single_pass;
  size_t off = 0;
  L.state_off = 0;
  off = round_up(sizeof(PcgState), 256);
  for (int s = 0; s < kHaloSlots; ++s) {
    L.peer[s] = sd.peer(s);
    // pcg2: one line of r per side; pcg1: 2 lines x (r, p) per side, one (r, p) per corner
    const int line = s < 2 ? sd.ny : sd.nx;
    L.edge_len[s] = single_pass ? (s < 4 ? 4 * line : 2) : (s < 4 ? line : 0);
    // s-step (packed, k_ca_halo): ca_gh lines x (z, p) per side, a ca_gh x ca_gh block per corner
    if (ca_gh > 0) L.edge_len[s] = 2 * ca_gh * (s < 4 ? line : ca_gh);
  }
  for (int s = 0; s < kHaloSlots; ++s) {
    L.send_off[s] = off;
    off = round_up(off + L.edge_len[s] * L.elem, 256);
  }
  for (int s = 0; s < kHaloSlots; ++s) {
    L.recv_off[s] = off;
    off = round_up(off + L.edge_len[s] * L.elem, 256);
  }
  L.bytes = off;
  return L;
}

GpuSubdomainSolver::GpuSubdomainSolver(const ProblemSpec& spec, const Subdomain& sd,
                                       const GpuOptions& opt, uintptr_t external_arena)
    : spec_(spec), sd_(sd), opt_(resolve_options(opt)), g_(spec) {
  spec.validate();
  PMX_CHECK(sd.nx >= 1 && sd.ny >= 1, "empty subdomain");
  apply_sigma_rules(spec_, sd_.grid, opt_);
  HIP_CHECK(hipSetDevice(opt_.device));
  construct(external_arena);  // if it throws, the members' owners free what it had allocated
}

void GpuSubdomainSolver::construct(uintptr_t external_arena) {
  const GpuOptions& opt = opt_;
  const ProblemSpec& spec = spec_;
  const Subdomain& sd = sd_;
  size_t free_b = 0, total_b = 0;
  HIP_CHECK(hipMemGetInfo(&free_b, &total_b));

  // iteration algorithm (see GpuOptions::algo); a Session resolves it once for all its solvers
  // (a standalone decomposed solver cannot know its transport: no s-step by auto there)
  if (opt_.algo == -1) opt_.algo = choose_algo(spec, sd.grid, opt_, double(total_b), 1, false);
  pcg1_ = opt_.algo == 1;
  ca_ = opt_.algo == 3;
  PMX_CHECK(!ca_ || (!opt.exact && sd.nx >= opt.ca_s && (sd.grid.Py == 1 || sd.ny >= opt.ca_s)),
            "s-step PCG (algo 3) runs the fast arithmetic, on subdomains of at least s rows (and s columns on "
            "2-D blocks)");
  // the s-step's fused pass (GpuOptions::ca_fuse) reads radius 2s: every subdomain must hold 2s rows (and
  // columns on 2-D blocks) -- decided from global data, so every rank runs the same schedule
  const bool fuse_ok = sd.grid.size() == 1 || ((spec.M - 1) / sd.grid.Px >= 2 * opt_.ca_s &&
                                               (sd.grid.Py == 1 || (spec.N - 1) / sd.grid.Py >= 2 * opt_.ca_s));
  PMX_CHECK(!ca_ || opt_.ca_fuse != 1 || fuse_ok, "the fused s-step pass needs subdomains of at least 2 s rows / columns");
  ca_fuse_ = ca_ && (opt_.ca_fuse == 1 || (opt_.ca_fuse == -1 && fuse_ok));
  // ghost rows per side: 2 (the single-pass radius-2 halo); a decomposed s-step subdomain needs s, 2s with
  // the fused pass (rows, and columns on 2-D blocks)
  const int gh = ca_ && sd.grid.size() > 1 ? (ca_fuse_ ? 2 * opt_.ca_s : opt_.ca_s) : 2;
  PMX_CHECK(!pcg1_ || (!opt.exact && (sd.grid.size() == 1 || (sd.nx >= 2 && sd.ny >= 2))),
            "pcg1 needs the fast arithmetic and a subdomain of at least 2 x 2 nodes");
  PMX_CHECK(!opt_.diffusion || (pcg1_ && opt_.shift_field), "a diffusion field runs pcg1 with the shift field");
  PMX_CHECK(!opt_.domain || opt_.diffusion, "a level-set domain runs the diffusion sweeps");
  plan_ = MemoryPlan(spec, sd, opt.dtype, opt_.algo, gh, opt_.shift_field != 0, opt_.diffusion != 0,
                     opt_.domain != 0);
  const int elem = int(plan_.elem);
  geom_ = make_dev_geom(spec, sd, plan_.pitch);
  const DevGeom& G = geom_;
  {  // fail with a sizing message instead of a bare hipErrorOutOfMemory
    const size_t need = estimate_device_bytes_algo(spec, sd, opt.dtype, opt_.algo) +
                        (plan_.nshift + plan_.ndiff) * plan_.field_bytes + plan_.diff_extra + plan_.mask_bytes;
    PMX_CHECK(need <= free_b,
              "subdomain " << sd.nx << "x" << sd.ny << " (" << (ca_ ? "s-step, 7" : pcg1_ ? "pcg1, 5" : "pcg2, 4")
                           << " fields) needs " << need / 1e9 << " GB on device " << opt.device
                           << " but only " << free_b / 1e9 << " of " << total_b / 1e9
                           << " GB are free; the largest square grid for this precision on one such "
                              "device is ~"
                           << max_square_grid(double(total_b), 1, opt.dtype) << "^2 (pmx --plan)");
  }
  // One allocation for all fields.  The offset between the fields (0 ... 8 MiB of stagger) and
  // physically contiguous memory were measured: no gain (profiles/r3/placement/stagger.log); where the
  // block lands is what matters (place_fields).
  fields_ = dev_alloc<char>(plan_.fields_total());
  if (const char* e = std::getenv("PMX_DEBUG_ALLOC"); e && e[0] == '1')
    std::fprintf(stderr, "pmx alloc: fields %p (%zu B, mod 1G %zu, mod 2M %zu)\n", static_cast<void*>(fields_.get()),
                 plan_.fields_total(), size_t(reinterpret_cast<uintptr_t>(fields_.get()) % (size_t(1) << 30)),
                 size_t(reinterpret_cast<uintptr_t>(fields_.get()) % (size_t(1) << 21)));

  // 1D face tables
  double* tables_buf = nullptr;
  tables_ = upload_tables(spec, &tables_buf);
  tables_buf_.reset(tables_buf);
  ca_geom_ = geom_;
  ca_tables_ = tables_;
  if (ca_ && opt_.ca_dirichlet) {  // see ca_tables_
    const int o = geom_.gi0;
    ca_geom_.nb = 0;
    ca_geom_.gi0 = 0;
    ca_geom_.M = sd.nx + 1;
    if (sd.grid.Py > 1) {  // 2-D blocks: also Dirichlet across y, on the problem's columns 1 .. ny
      ca_geom_.gj0 = 0;
      ca_geom_.N = sd.ny + 1;
    }
    for (const double** t : {&ca_tables_.rv, &ca_tables_.xlo, &ca_tables_.xhi, &ca_tables_.x}) *t += o;
    ca_tables_.acls += 4 * o;
    ca_tables_.bcls += 4 * o;
  }
  ca_gh_ = ca_geom_.nb ? gh : 2;

  // tile shapes per kernel (profiles/tile_counters_16384_fp64.md: pcg_a is fastest with 4
  // columns/lane, pcg_b with 2 in fp64; fp32 moves 16 B with 4 columns)
  const bool fp64 = elem == 8;
  const int vec_a = opt.vec ? opt.vec : (opt.waves == 4 ? 4 : 2);  // (4, 4) is instantiated
  const int vec_b = opt.vec_b ? opt.vec_b : opt.vec ? opt.vec : (fp64 || opt.waves != 4 ? 2 : 4);
  const int waves_b = opt.waves_b ? opt.waves_b : opt.waves;
  const int rows_b = opt.tile_rows_b >= 0 ? opt.tile_rows_b : opt.tile_rows;
  // auto tile heights (caps and tile-count targets from bench/tile_sweep.py, see make_wave_tiles)
  tiles_ = make_wave_tiles(G, vec_a, opt.waves, opt.tile_rows, 32, 22000);
  if (opt.b_ring)
    tiles_b_ = make_wave_tiles(G, vec_b, waves_b, rows_b, 24, 66000);
  else  // default: ring-free 2-row tiles, independent of the pcg_a height
    tiles_b_ = make_row_tiles(G, vec_b, waves_b, opt.tile_rows_b >= 0 ? opt.tile_rows_b : 0);
  tiles_b_.pair_w = tiles_b_.kind == 2 && !opt.exact && opt_.pair_w != 0;

  if (pcg1_) {
    // block tiles (pcg1_block.hip): undecomposed fp64 grids, the three pipeline stages row-parallel
    // across a workgroup's 8 waves.  Auto where the march is latency-bound, by its four-row tile
    // count T4 (study r4ac, profiles/r4/block/, us/iteration block vs march): T4 < 1000 8-row tiles
    // (400x600 17.3 vs 37.1), T4 < 10000 12-row tiles (800x1200 23.9 vs 42.0, 1200x1800 39.1 vs
    // 54.1, 1600x2400 59.9 vs 61.2); above, the march (2000x3000 85.7 vs 76.1).  PMX_PCG1_BLOCK=0/1
    // forces it, PMX_PCG1_BLOCK_ROWS=4|8|12|16 and PMX_PCG1_BLOCK_WAVES=8|16 pick the shape.
    const int blk = opt_.block1;
    const int64_t t4 = int64_t((G.nx + 3) / 4) * ((G.ny + 123) / 124);
    if (G.nb == 0 && elem == 8 && (blk == 1 || (blk == -1 && t4 < 10000))) {
      const int rows = opt_.block_rows1 ? opt_.block_rows1 : t4 < 1000 ? 8 : 12;
      PMX_CHECK(pcg1_block_shape_ok(rows, opt_.block_waves1),
                "block tiles: no " << rows << "-row x " << opt_.block_waves1 << "-wave variant");
      block1_ = true;
      // the reduction folded into the sweep costs every workgroup a drain of its stores and a ticket
      // round trip while it holds its LDS: cheaper than a k_reduce_n launch when the tiles run in
      // about one round (400x600 16.8 vs 18.3 us, 800x1200 23.3 vs 24.6), dearer over several
      // (1200x1800 37.5 vs 37.2, 1600x2400 57.3 vs 54.9; study r4ap).  PMX_PCG1_BLOCK_FUSED=0/1 forces it.
      const int64_t nblk = int64_t((G.nx + rows - 1) / rows) * ((G.ny + 123) / 124);
      block_fused_ = opt_.block_fused1 >= 0 ? opt_.block_fused1 == 1 : nblk < 1500;
      opt_.rows1 = rows;
      opt_.rows1w = rows;
      opt_.vec1 = 2;
      opt_.waves1 = 1;
      opt_.waves1w = 1;
      opt_.pf1 = opt_.pf1w = 1;
    }
    tiles1_ = make_pcg1_tiles(G, opt_.vec1, opt_.waves1, opt_.rows1, opt_.pf1, elem);
#ifdef PMX_WAVE_TRACE
    if (const char* e = std::getenv("PMX_WAVE_TRACE_IT"); e && e[0]) {
      wtrace_n_ = tiles1_.ntiles();
      wtrace_ = pcg1_wave_trace_setup(std::atoll(e), wtrace_n_);
    }
#endif
    // (a diffusion session runs fp64 registers on fp32 storage too: no packed-fp32 diffusion sweep is built)
    tiles1_.arith32 = elem == 4 && opt_.arith32 && !opt_.diffusion ? 1 : 0;
    const int waves_w = opt_.waves1w ? opt_.waves1w : (opt_.waves1 == 8 ? 4 : opt_.waves1);
    tiles1w_ = make_pcg1_tiles(G, opt_.vec1, waves_w, opt_.rows1w ? opt_.rows1w : tiles1_.rows,
                               opt_.pf1w ? opt_.pf1w : tiles1_.pf, elem);
    tiles1w_.arith32 = tiles1_.arith32;
    tiles1_.lds_pad = pcg1_lds_pad(opt_.wpcu1, tiles1_.waves);
    tiles1w_.lds_pad = pcg1_lds_pad(opt_.wpcu1w, tiles1w_.waves);
    if (block1_) tiles1_.bwaves = tiles1w_.bwaves = opt_.block_waves1;
    // the LDS-DMA march: fp64 with the default shape only (VEC 2, 1 wave, register prefetch 1)
    auto dma_ok = [&](const TileCfg& t) { return elem == 8 && t.vec == 2 && t.waves == 1 && t.pf == 1; };
    if (dma_ok(tiles1_)) tiles1_.dpf = opt_.dma1;
    if (dma_ok(tiles1w_)) tiles1w_.dpf = opt_.dma1w >= 0 ? opt_.dma1w : opt_.dma1;
    const bool same_w = tiles1w_.rows == tiles1_.rows && tiles1w_.waves == tiles1_.waves;
    // dispatch order tables with the tiles' row classes; order1: the ellipse-cut tiles first
    // within each XCD's share (their 3-5x longer tiles would trail the sweep)
    tile_order_ = dev_alloc<Pcg1Slot>(pcg1_order_slots(tiles1_) * sizeof(Pcg1Slot));
    slow_tiles_ = pcg1_build_order(G, tables_, tiles1_, tile_order_.get(), opt_.order1 != 0, nullptr);
    if (same_w) {
      tiles1w_.order0 = tiles1_.order0;
      tiles1w_.order1 = tiles1_.order1;
      tiles1w_.order2 = tiles1_.order2;
      for (int q = 0; q < 3; ++q) tiles1w_.groups[q] = tiles1_.groups[q];
    } else {
      tile_order_w_ = dev_alloc<Pcg1Slot>(pcg1_order_slots(tiles1w_) * sizeof(Pcg1Slot));
      (void)pcg1_build_order(G, tables_, tiles1w_, tile_order_w_.get(), opt_.order1 != 0, nullptr);
    }
  }

  if (ca_) {
    ca_tiles_ = make_ca_tiles(ca_geom_, opt_.ca_s, opt_.ca_rows, opt_.ca_rows2, opt_.ca_rows_f);
    ca_tiles_.fuse = ca_fuse_ ? 1 : 0;
    if (const char* e = study_env("PMX_CA_SPLIT_F"); e && e[0]) ca_tiles_.split_f = std::atoi(e);
    // the face coefficients of every node, read on the rows the ellipse cuts (2 more field-sized arrays)
    // fp64 whatever the fields' storage, in the fields' pitch (elements); column 1 of every row 256-B aligned
    ca_faces_ = dev_alloc<char>(plan_.faces_total());
    ca_tiles_.fa = reinterpret_cast<const double*>(ca_faces_.get() + plan_.face_at(0));
    ca_tiles_.fb = reinterpret_cast<const double*>(ca_faces_.get() + plan_.face_at(1));
    ca_tiles_.gh = ca_gh_;
    ca_build_faces(ca_geom_, ca_tables_, const_cast<double*>(ca_tiles_.fa), const_cast<double*>(ca_tiles_.fb), ca_gh_, nullptr);
    const bool split = opt_.ca_split == -1 ? geom_.nb != 0 : opt_.ca_split == 1;  // see GpuOptions::ca_split
    if (!split) ca_tiles_.split = 0;
    ca_tiles_.dma = elem == 8 ? (opt_.ca_dma == -1 ? int(split) : opt_.ca_dma) : 0;  // LDS-DMA rows: fp64
    if (ca_tiles_.split && opt_.ca_frame_stream) {
      ca_side_ = make_stream();
      ca_ev_fork_ = make_event(hipEventDisableTiming);
      ca_ev_join_ = make_event(hipEventDisableTiming);
    }
    ca_tbl_ = dev_alloc<unsigned>(size_t(ca_tiles_.tiles_j) * ca_tiles_.cwords * sizeof(unsigned));
    ca_tiles_.tbl = ca_tbl_.get();
    ca_build_classes(ca_geom_, ca_tables_, ca_tiles_, ca_tbl_.get(), nullptr);
    if (ca_tiles_.fuse) {
      ca_tbl_f_ = dev_alloc<unsigned>(size_t(ca_tiles_.tiles_j_f) * ca_tiles_.cwords * sizeof(unsigned));
      ca_tiles_.tbl_f = ca_tbl_f_.get();
      ca_build_classes(ca_geom_, ca_tables_, ca_tiles_, ca_tbl_f_.get(), nullptr, true);
    }
    HIP_CHECK(hipStreamSynchronize(nullptr));
    ca_state_ = dev_alloc<CaState>(sizeof(CaState));
    HIP_CHECK(hipMemset(ca_state_.get(), 0, sizeof(CaState)));
    ca_chunk_ = dev_alloc<double>(size_t(kCaReduceMaxBlocks) * ca_nq(ca_tiles_.s) * sizeof(double));
  }
  init_tiles_ = make_tiles(G, 256, 0);
  // partials: 5 doubles per slot (the s-step Gram partials take ca_nq per tile)
  const int ca_slots =
      ca_ ? int((std::max(int64_t(ca_tiles_.ntiles()) * (ca_nq(ca_tiles_.s) - ca_tiles_.s) +
                              int64_t(ca_tiles_.ntiles2()) * ca_tiles_.s,
                          int64_t(ca_tiles_.fuse ? ca_tiles_.ntilesf() : 0) * ca_nq(ca_tiles_.s)) + 4) / 5)
          : 0;
  const size_t npart = size_t(std::max({tiles_.ntiles(), tiles_b_.ntiles(), init_tiles_.ntiles(),
                                        pcg1_ ? std::max(tiles1_.ntiles(), tiles1w_.ntiles()) : 0, ca_slots}));
  npart_ = npart;
  partials_ = dev_alloc<double>((npart * 5 + kReduceWsDoubles) * sizeof(double));
  reduce_ws_ = partials_.get() + npart * 5;
  HIP_CHECK(hipMemset(reduce_ws_, 0, kReduceWsDoubles * sizeof(double)));

  layout_ = comm_layout(sd, opt.dtype, pcg1_ || ca_, ca_ && sd.grid.size() > 1 ? gh : 0);
  if (external_arena) {
    arena_ = reinterpret_cast<char*>(external_arena);
    PMX_CHECK(external_arena % 256 == 0, "external comm arena must be 256-B aligned");
  } else {
    arena_own_ = dev_alloc<char>(layout_.bytes);
    arena_ = arena_own_.get();
  }
  HIP_CHECK(hipMemset(arena_, 0, layout_.bytes));
  state_ = reinterpret_cast<PcgState*>(arena_ + layout_.state_off);
  host_state_ = host_alloc<PcgState>(2 * sizeof(PcgState), hipHostMallocDefault);
  if (opt_.progress) {
    progress_host_ = host_alloc<long long>(64, hipHostMallocMapped | hipHostMallocCoherent);
    std::memset(progress_host_.get(), 0, 64);
    void* d = nullptr;
    HIP_CHECK(hipHostGetDevicePointer(&d, progress_host_.get(), 0));
    progress_dev_ = static_cast<long long*>(d);
  }
  if (pcg1_ || ca_) place_fields();
}

// Field placement probe.  On MI355X the same sweep runs at one of (at least) three rates depending
// on WHERE its fields were allocated: a property of the allocation, stable for its lifetime and
// across passes (8 sessions alive in one process, timed forward then in reverse).  At 16384^2 fp64,
// 3 plain sweeps of a candidate block take ~5.45, ~4.97 or ~4.55-4.63 ms, and the iteration runs
// at ~2150 / ~1995 / ~1810 us -- profiles/r3/placement/, profiles/r4/placement/.  So the solver may
// allocate candidate blocks and keep the fastest: at most opt.placement of them (GpuOptions), while
// opt.placement_keep_free of the memory that was free stays free and for at most
// opt.placement_budget_s seconds of timing; blocks under 256 MB are not probed (latency-bound
// grids).  Each candidate: 6 real iterations (probe_iterations; init() resets everything afterwards).
// Construction time only; nothing in the iteration changes.  Off by default (the library) and for
// ranks that share a device; skipped with an external (IPC-shared) arena.
// One candidate's rate: the iteration itself, in its real buffer roles -- init, two untimed
// iterations, then 6 timed ones (a whole parity x w-cycle period: plain and w sweeps with r / r2 and
// p0 / p1 in both assignments).  Round 4: the earlier probe (3 plain sweeps with the fields in
// rotating roles) ranked blocks whose iteration rates differ by 7% within 1% of each other
// (profiles/r4/placement/).  No ghost exchange (timing only); the driver's init() resets everything.
void GpuSubdomainSolver::probe_iterations(hipStream_t s, hipEvent_t e0, hipEvent_t e1) {
  enqueue_init(s);
  if (ca_ && ca_fused()) {  // fused schedule: pass 1 + reduction untimed, then two fused blocks -- the
    // kernels a solve actually runs (pass 1 / pass 2 rank blocks differently from the fused pass:
    // round 6, a probe of the unfused passes kept blocks on which the fused pass ran ~6% slower)
    enqueue_ca_pass(s, false);
    enqueue_ca_reduce(s, ca_tiles_.s, false, true);
    HIP_CHECK(hipEventRecord(e0, s));
    for (int k = 0; k < 2; ++k) {
      enqueue_ca_fused(s);
      enqueue_ca_reduce(s, ca_tiles_.s, false, true, true);
    }
    HIP_CHECK(hipEventRecord(e1, s));
    return;
  }
  if (ca_) {  // s-step: one untimed block, then two (2 s iterations); strips: this rank's sums only
    const auto block = [&] {
      enqueue_ca_pass(s, false);
      enqueue_ca_reduce(s, ca_tiles_.s, false, true);
      enqueue_ca_pass(s, true);
    };
    block();
    HIP_CHECK(hipEventRecord(e0, s));
    for (int k = 0; k < 2; ++k) block();
    HIP_CHECK(hipEventRecord(e1, s));
    return;
  }
  for (int k = 0; k < 2; ++k) enqueue_phase_a(s);
  HIP_CHECK(hipEventRecord(e0, s));
  for (int k = 0; k < 6; ++k) enqueue_phase_a(s);
  HIP_CHECK(hipEventRecord(e1, s));
}

void GpuSubdomainSolver::place_fields() {
  const int K = opt_.placement;
  const size_t block = plan_.fields_total();
  if (K <= 1 || !arena_own_ || block < (size_t(256) << 20)) return;  // small grids: latency-bound
  const double t0 = now_s();
  // candidate blocks; fields_ holds candidate `cur`, whose slot is empty meanwhile
  std::vector<DevPtr<char>> cand(1);
  size_t cur = 0;
  auto use = [&](size_t c) {
    cand[cur] = std::move(fields_);
    fields_ = std::move(cand[c]);
    cur = c;
  };
  size_t free0 = 0, total_b = 0;
  HIP_CHECK(hipMemGetInfo(&free0, &total_b));
  const size_t keep = std::max(size_t(double(free0) * std::clamp(opt_.placement_keep_free, 0.0, 1.0)),
                               size_t(4) << 30);
  while (int(cand.size()) < K) {
    size_t free_b = 0;
    HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    if (free_b < block + keep) break;
    char* p = nullptr;
    if (hipMalloc(&p, block) != hipSuccess) {
      (void)hipGetLastError();
      break;
    }
    cand.emplace_back(p);
  }
  if (cand.size() == 1) {
    placement_s_ = now_s() - t0;
    return;
  }
  // the time budget bounds the timed sweeps; allocation (the driver clears reused VRAM) is reported
  // in placement_seconds but not charged to it
  const double t_probe = now_s();
  const Stream s = make_stream();
  const Event e0 = make_event(), e1 = make_event();
  try {
    placement_ms_.clear();
    for (size_t c = 0; c < cand.size(); ++c) {
      if (c > 0 && now_s() - t_probe > opt_.placement_budget_s) break;  // time budget: the rest stay untimed
      placement_ms_.push_back(0.f);
      use(c);
      probe_iterations(s.get(), e0.get(), e1.get());
      HIP_CHECK(hipEventSynchronize(e1.get()));
      HIP_CHECK(hipEventElapsedTime(&placement_ms_[c], e0.get(), e1.get()));
    }
  } catch (...) {  // keep the first block (the solver's own), then report; `cand` frees the others
    (void)hipStreamSynchronize(s.get());
    use(0);
    placement_ms_.clear();
    throw;
  }
  const auto pick = opt_.placement_pick == 1 ? std::max_element(placement_ms_.begin(), placement_ms_.end())
                                             : std::min_element(placement_ms_.begin(), placement_ms_.end());
  use(size_t(pick - placement_ms_.begin()));
  cand.clear();  // the other candidates
  placement_s_ = now_s() - t0;
}

void GpuSubdomainSolver::progress(long long out[3]) const {
  for (int q = 0; q < 3; ++q)
    out[q] = progress_host_ ? __atomic_load_n(progress_host_.get() + q, __ATOMIC_RELAXED) : -1;
}

// Paired w updates (k_pcg_b_rows): an odd iteration leaves w^{k+1} = w^k + alpha_k p^k pending in device
// memory.  pcg1 (k_pcg1) leaves w_pend_n (1 or 2) steps pending, p^j in p[j & 1], alpha_j in alpha1[j & 3].
GpuSubdomainSolver::PendingW GpuSubdomainSolver::pending_w(const PcgState& st) const {
  PendingW pw;
  if (pcg1_ && st.w_pend_n > 0 && st.w_pend > 0) {
    pw.n = st.w_pend_n;
    for (int q = 0; q < pw.n; ++q) {  // q = 0: the oldest pending step
      const long long j = st.w_pend - (pw.n - 1) + q;
      pw.field[q] = (j & 1) ? 3 : 2;
      pw.a[q] = st.alpha1[j & 3];
    }
  } else if (!pcg1_ && st.w_pend > 0) {
    pw.n = 1;
    pw.field[0] = (st.w_pend & 1) ? 3 : 2;
    pw.a[0] = st.alpha[st.w_pend & 1];
  }
  return pw;
}

namespace {
// rows x cols doubles with row stride ld -> the storage type, dense
std::vector<char> round_to_storage(const double* v, size_t rows, size_t cols, size_t ld, size_t elem) {
  std::vector<char> out(rows * cols * elem);
  for (size_t i = 0; i < rows; ++i) {
    const double* src = v + i * ld;
    if (elem == 8) {
      std::memcpy(out.data() + i * cols * 8, src, cols * 8);
    } else {
      float* o = reinterpret_cast<float*>(out.data()) + i * cols;
      for (size_t k = 0; k < cols; ++k) o[k] = static_cast<float>(src[k]);
    }
  }
  return out;
}
}  // namespace

void GpuSubdomainSolver::set_init_data(const double* f, const double* w0, int64_t ld_f, int64_t ld_w0) {
  const size_t nx = size_t(sd_.nx), ny = size_t(sd_.ny);
  stage_f_ = f ? round_to_storage(f, nx, ny, ld_f ? size_t(ld_f) : ny, plan_.elem) : std::vector<char>();
  stage_w_ = w0 ? round_to_storage(w0, nx + 2, ny + 2, ld_w0 ? size_t(ld_w0) : ny + 2, plan_.elem) : std::vector<char>();
  dev_f_ = dev_w_ = nullptr;  // each call replaces the data of the next init
}

void GpuSubdomainSolver::set_reaction(const double* c, int64_t ld, bool on_device, hipStream_t s) {
  PMX_CHECK(has_shift_field(), "set_reaction needs a solver built with a shift field (GpuOptions::shift_field)");
  PMX_CHECK(c && ld >= spec_.N + 1, "set_reaction needs an (M+1) x (N+1) array with row stride >= N+1");
  HIP_CHECK(hipSetDevice(opt_.device));
  // the block with its radius-2 frame (local rows -1 .. nx+2, columns -1 .. ny+2), clipped to the interior
  // nodes of the box; everything else of the field is 0
  const int gi_lo = std::max(1, sd_.gi0() - 1), gi_hi = std::min(spec_.M - 1, sd_.gi0() + sd_.nx + 2);
  const int gj_lo = std::max(1, sd_.gj0() - 1), gj_hi = std::min(spec_.N - 1, sd_.gj0() + sd_.ny + 2);
  const int rows = gi_hi - gi_lo + 1, cols = gj_hi - gj_lo + 1;
  const int f = plan_.shift_field();
  const double* src = c + int64_t(gi_lo) * ld + gj_lo;
  char* dst = field_ptr(f, gi_lo - sd_.gi0(), gj_lo - sd_.gj0());
  HIP_CHECK(hipMemsetAsync(field_raw(f), 0, plan_.field_bytes, s));
  std::vector<char> stage;  // the host path: T(sigma + c), dense, until s has copied it
  if (on_device) {
    with_storage([&](auto t) {
      using T = decltype(t);
      launch_scatter_shift<T>(src, ld, reinterpret_cast<T*>(dst), plan_.pitch, rows, cols, spec_.sigma, s);
    });
  } else {
    stage.resize(size_t(rows) * size_t(cols) * plan_.elem);
    with_storage([&](auto t) {
      using T = decltype(t);
      T* o = reinterpret_cast<T*>(stage.data());
      for (int i = 0; i < rows; ++i)
        for (int j = 0; j < cols; ++j) o[size_t(i) * cols + j] = static_cast<T>(spec_.sigma + src[int64_t(i) * ld + j]);
    });
    HIP_CHECK(hipMemcpy2DAsync(dst, plan_.row_bytes(), stage.data(), size_t(cols) * plan_.elem, size_t(cols) * plan_.elem,
                               size_t(rows), hipMemcpyHostToDevice, s));
  }
  HIP_CHECK(hipStreamSynchronize(s));
}

void GpuSubdomainSolver::set_diffusion(const double* k, int64_t ld, hipStream_t s) {
  PMX_CHECK(has_diffusion(), "set_diffusion needs a solver built with a diffusion field (GpuOptions::diffusion)");
  PMX_CHECK(k && ld >= spec_.N + 1, "set_diffusion needs an (M+1) x (N+1) device array with row stride >= N+1");
  HIP_CHECK(hipSetDevice(opt_.device));
  with_storage([&](auto t) {
    using T = decltype(t);
    launch_face_fields<T>(geom_, tables_, k, ld, reinterpret_cast<T*>(field_ptr(plan_.diff_field(0))),
                          reinterpret_cast<T*>(field_ptr(plan_.diff_field(1))), s);
  });
  HIP_CHECK(hipStreamSynchronize(s));
}

void GpuSubdomainSolver::set_domain(const double* phi, int64_t ldp, const double* k, int64_t ld, hipStream_t s) {
  PMX_CHECK(has_domain(), "set_domain needs a solver built with a level-set domain (GpuOptions::domain)");
  PMX_CHECK(phi && ldp >= spec_.N + 1 && (!k || ld >= spec_.N + 1),
            "set_domain needs (M+1) x (N+1) device arrays with row stride >= N+1");
  HIP_CHECK(hipSetDevice(opt_.device));
  with_storage([&](auto t) {
    using T = decltype(t);
    launch_domain_fields<T>(geom_, phi, ldp, k, ld, reinterpret_cast<T*>(field_ptr(plan_.diff_field(0))),
                            reinterpret_cast<T*>(field_ptr(plan_.diff_field(1))),
                            reinterpret_cast<unsigned char*>(fields_.get() + plan_.mask_off()), s);
  });
  HIP_CHECK(hipStreamSynchronize(s));
}

void GpuSubdomainSolver::set_init_data_device(const double* f, const double* w0, int64_t ld_f, int64_t ld_w0) {
  PMX_CHECK(!f || ld_f >= sd_.ny, "row stride of the device right-hand side below the block's width");
  PMX_CHECK(!w0 || ld_w0 >= sd_.ny + 2, "row stride of the device initial guess below the block's width");
  if (f) {
    std::vector<char>().swap(stage_f_);
    dev_f_ = f;
    dev_ld_f_ = ld_f;
  }
  if (w0) {
    std::vector<char>().swap(stage_w_);
    dev_w_ = w0;
    dev_ld_w_ = ld_w0;
  }
}

double GpuSubdomainSolver::residual_sumsq(const double* f, hipStream_t s, int64_t ld_f, bool f_on_device) const {
  HIP_CHECK(hipSetDevice(opt_.device));
  PMX_CHECK(!(f && f_on_device) || ld_f >= sd_.ny, "a device right-hand side needs its row stride");
  const PendingW pw = pending_w(read_state(s));
  // temporary device memory for the call: one partial pair per init tile, and f in the storage type
  // (a device f in fp64 storage is read where it lies)
  const size_t nt = size_t(init_tiles_.ntiles()), elem = plan_.elem;
  const bool host_f = f && !f_on_device, in_place = f && f_on_device && elem == 8;
  const std::vector<char> hf =
      host_f ? round_to_storage(f, size_t(sd_.nx), size_t(sd_.ny), ld_f ? size_t(ld_f) : size_t(sd_.ny), elem)
             : std::vector<char>();
  const size_t fbytes = f && !in_place ? size_t(sd_.nx) * size_t(sd_.ny) * elem : 0;
  const DevPtr<char> tmp = dev_alloc<char>(2 * nt * sizeof(double) + fbytes);
  double* part = reinterpret_cast<double*>(tmp.get());
  char* tmp_f = tmp.get() + 2 * nt * sizeof(double);
  const void* df = !f ? nullptr : in_place ? static_cast<const void*>(f) : tmp_f;
  const int64_t fpitch = in_place ? ld_f : sd_.ny;
  std::vector<double> h(2 * nt);
  if (host_f) HIP_CHECK(hipMemcpyAsync(tmp_f, hf.data(), hf.size(), hipMemcpyHostToDevice, s));
  if (f && f_on_device && !in_place)
    launch_scatter<float>(f, ld_f, reinterpret_cast<float*>(tmp_f), sd_.ny, sd_.nx, sd_.ny, s);
  with_storage([&](auto t) {
    using T = decltype(t);
    InitData<T> X;
    // f is nx x ny with row stride fpitch: element (i, j), i, j >= 1, at f[(i - 1) * fpitch + (j - 1)]
    X.f = df ? static_cast<const T*>(df) - (fpitch + 1) : nullptr;
    X.fpitch = fpitch;
    X.pa = pending_p<T>(pw, 0);
    X.pb = pending_p<T>(pw, 1);
    X.ca = pw.a[0];
    X.cb = pw.a[1];
    X.npend = pw.n;
    set_operator(X, op<T>());
    X.mask = mask_base();
    launch_init_data<T>(geom_, tables_, fields<T>().w, nullptr, HaloBufs<T>{}, part, init_tiles_, X, true, s);
  });
  HIP_CHECK(hipMemcpyAsync(h.data(), part, h.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  double sum = 0.0;
  for (size_t t = 0; t < nt; ++t) sum += h[2 * t + 1];  // tile order: deterministic
  return sum;
}

ErrorStats GpuSubdomainSolver::error_norms(hipStream_t s) const {
  HIP_CHECK(hipSetDevice(opt_.device));
  const PendingW pw = pending_w(read_state(s));  // pending w steps, exactly as download_w applies them
  constexpr int kMaxBlocks = 1024;
  const DevPtr<double> d_out = dev_alloc<double>(3 * kMaxBlocks * sizeof(double));
  const int nb = with_storage([&](auto t) {
    using T = decltype(t);
    return launch_error_norms<T>(geom_, tables_, fields<T>().w, pending_p<T>(pw, 0), pw.a[0], pending_p<T>(pw, 1),
                                 pw.a[1], pw.n, d_out.get(), kMaxBlocks, s);
  });
  std::vector<double> h(3 * size_t(nb));
  HIP_CHECK(hipMemcpyAsync(h.data(), d_out.get(), h.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  ErrorStats e;
  e.max_w = -HUGE_VAL;
  for (int b = 0; b < nb; ++b) {  // block order: deterministic
    e.sum_e2 += h[3 * size_t(b)];
    e.max_e = std::max(e.max_e, h[3 * size_t(b) + 1]);
    e.max_w = std::max(e.max_w, h[3 * size_t(b) + 2]);
  }
  return e;
}

GpuSubdomainSolver::~GpuSubdomainSolver() {
#ifdef PMX_WAVE_TRACE
  if (wtrace_) {  // one line per wave: start end xcc hw_id tile part prologue_end (100 MHz ticks)
    std::vector<unsigned long long> h(size_t(wtrace_n_) * 5);
    if (hipMemcpy(h.data(), wtrace_, h.size() * 8, hipMemcpyDeviceToHost) == hipSuccess) {
      const char* fn = std::getenv("PMX_WAVE_TRACE_OUT");
      if (FILE* f = std::fopen(fn && fn[0] ? fn : "wave_trace.txt", "w")) {
        for (int b = 0; b < wtrace_n_; ++b) {
          const unsigned long long* o = &h[size_t(b) * 5];
          if (o[1]) std::fprintf(f, "%llu %llu %llu %llu %llu %llu %llu\n", o[0], o[1], o[2] >> 32, o[2] & 0xffffffffull,
                                 o[3] & 0xffffffffffull, o[3] >> 40, o[4]);
        }
        std::fclose(f);
      }
    }
    (void)hipFree(wtrace_);
  }
#endif
  // the device idle, then the members' owners free everything (an external arena is not owned)
  (void)hipSetDevice(opt_.device);
  (void)hipDeviceSynchronize();
}

size_t GpuSubdomainSolver::estimate_device_bytes_algo(const ProblemSpec& spec, const Subdomain& sd, DType dtype,
                                                      int algo) {
  // s-step on decomposed grids: the most ghost rows a solver may choose (2s = 6: the fused pass)
  const int gh = algo == 3 && sd.grid.size() > 1 ? 2 * kCaMaxS : 2;
  const MemoryPlan plan(spec, sd, dtype, algo, gh);
  // partials: at most one per 2 rows x 64 columns tile (the smallest auto tile), 5 doubles each; the
  // s-step: 21 doubles per 8-row tile of 116 columns (the smallest tiling), row-class words
  const size_t partials = algo == 3 ? (size_t(sd.nx) / 8 + 1) * (size_t(sd.ny) / 116 + 1) * 21 * 8 * 2
                                    : (size_t(sd.nx + 1) / 2 + 1) * (size_t(sd.ny) / 64 + 1) * 40;
  return plan.total() + partials + comm_layout(sd, dtype, algo == 1 || algo == 3, algo == 3 && sd.grid.size() > 1 ? gh : 0).bytes +
         (1u << 20);
}

size_t GpuSubdomainSolver::device_bytes() const {
  return plan_.total() + (npart_ * 5 + kReduceWsDoubles) * sizeof(double) + (arena_own_ ? layout_.bytes : 0);
}

void* GpuSubdomainSolver::field_base(int which) const {
  PMX_CHECK(which >= 0 && which < 4, "field index");
  return field_ptr(which);
}

template <typename T>
HaloBufs<T> GpuSubdomainSolver::halo() const {
  HaloBufs<T> H;
  for (int s = 0; s < kHaloSlots; ++s) {
    H.send[s] = reinterpret_cast<T*>(arena_ + layout_.send_off[s]);
    H.recv[s] = reinterpret_cast<T*>(arena_ + layout_.recv_off[s]);
  }
  return H;
}

void GpuSubdomainSolver::after_launch(hipStream_t s) const {
  if (opt_.check) {
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(s));
  }
}

template <typename T>
void GpuSubdomainSolver::init_impl(hipStream_t s) {
  for (int f = 0; f < plan_.nfields; ++f) HIP_CHECK(hipMemsetAsync(field_raw(f), 0, plan_.field_bytes, s));
  HIP_CHECK(hipMemsetAsync(arena_, 0, layout_.bytes, s));
  PcgState& st = host_state_.get()[1];  // template (never rewritten while a copy is in flight)
  std::memset(&st, 0, sizeof(st));
  st.delta = spec_.delta;
  st.bd_tol = spec_.breakdown_tol;
  st.it = pcg1_ || ca_ ? 0 : 1;  // pcg1: sweep 0 (enqueued by the driver) forms (z^0, r^0), (A z^0, z^0)
  st.halo_k = 0;          // pcg1: the first ghost exchange fills sweep 0's inputs
  st.max_iter = spec_.effective_max_iter();
  st.norm = int(spec_.norm);
  st.pair_w = opt_.pair_w ? 1 : 0;
  st.pair_min_beta = opt_.pair_w == 2 ? HUGE_VAL : 1e-3;
  // The screened problem converges fast, so its beta_k are small (sigma = 1e4: 0.04 .. 0.2), and the
  // recovered p^{k-2} carries the STORAGE rounding of p^{k-1} and r^{k-1} times 1 / beta_{k-1}: with fp32
  // fields w then misses the oracle by 2.7e-6 max|w| where re-reading p^{k-2} gives 7e-8 (measured, 40x40
  // and 97x130, constant rhs).  There the sweep re-reads below beta = 0.5 (growth <= 3 roundings).
  if ((spec_.sigma != 0.0 || has_shift_field()) && sizeof(T) == 4 && opt_.pair_w != 2) st.pair_min_beta = 0.5;
  st.w_cycle = w_cycle();
  // stop rule: the step rule leaves PcgState's tail zero, as every build before it did
  stop_ref_data_ = false;
  if (spec_.stop == StopRule::kResidual) {
    stop_ref_data_ = !stage_w_.empty() || dev_w_ != nullptr;  // w0 given: the init reduces rho_B from the data
    st.stop = int(StopRule::kResidual);
    st.stop_flags = (stop_ref_data_ ? kStopRefData : 0) | (pcg1_ ? kStopRhoC : 0);
    st.rtol = spec_.rtol;
    st.atol = spec_.atol;
  }
  host_k_ = st.it;
  if (progress_host_) {  // the device has finished with them: init follows a synchronised state
    for (int q = 0; q < 3; ++q) __atomic_store_n(progress_host_.get() + q, 0LL, __ATOMIC_RELAXED);
  }
  HIP_CHECK(hipMemcpyAsync(state_, &st, sizeof(PcgState), hipMemcpyHostToDevice, s));
  const Fields<T> F = fields<T>();
  T *w = F.w, *r = F.r;
  // k_init packs r^0 into the two-sweep send buffers; pcg1 packs its own radius-2 halo
  DevGeom G = geom_;
  if (pcg1_) G.nb = 0;
  if (has_init_data()) {
    // user data (set_init_data), after the memsets above: f into r's owned nodes, w0 into w's owned
    // nodes and ring; r <- B - A w0; then w's ring is zero again, as every later kernel and the
    // checkpoints expect of w's ghosts
    const size_t P = size_t(geom_.pitch) * sizeof(T), nx = size_t(sd_.nx), ny = size_t(sd_.ny);
    InitData<T> X;
    X.fpitch = geom_.pitch;
    X.has_f = !stage_f_.empty() || dev_f_;
    X.has_w = !stage_w_.empty() || dev_w_;
    set_operator(X, op<T>());
    X.mask = mask_base();
    X.rho_b = stop_ref_data_ ? 1 : 0;
    // the same cells from either source: a staged host copy, or the caller's device block through the
    // scatter kernel (set_init_data_device)
    if (dev_f_)
      launch_scatter<T>(dev_f_, dev_ld_f_, r + geom_.pitch + 1, geom_.pitch, sd_.nx, sd_.ny, s);
    else if (X.has_f)
      HIP_CHECK(hipMemcpy2DAsync(r + geom_.pitch + 1, P, stage_f_.data(), ny * sizeof(T), ny * sizeof(T), nx,
                                 hipMemcpyHostToDevice, s));
    if (dev_w_)
      launch_scatter<T>(dev_w_, dev_ld_w_, w, geom_.pitch, sd_.nx + 2, sd_.ny + 2, s);
    else if (X.has_w)
      HIP_CHECK(hipMemcpy2DAsync(w, P, stage_w_.data(), (ny + 2) * sizeof(T), (ny + 2) * sizeof(T), nx + 2,
                                 hipMemcpyHostToDevice, s));
    launch_init_data<T>(G, tables_, w, r, halo<T>(), partials_.get(), init_tiles_, X, false, s);
    after_launch(s);
    if (X.has_w) {
      HIP_CHECK(hipMemsetAsync(w, 0, (ny + 2) * sizeof(T), s));
      HIP_CHECK(hipMemsetAsync(w + (nx + 1) * size_t(geom_.pitch), 0, (ny + 2) * sizeof(T), s));
      HIP_CHECK(hipMemset2DAsync(w + geom_.pitch, P, 0, sizeof(T), nx, s));
      HIP_CHECK(hipMemset2DAsync(w + geom_.pitch + ny + 1, P, 0, sizeof(T), nx, s));
    }
    HIP_CHECK(hipStreamSynchronize(s));  // the staged host copies / the caller's device blocks are read until here
    std::vector<char>().swap(stage_f_);
    std::vector<char>().swap(stage_w_);
    dev_f_ = dev_w_ = nullptr;
  } else {
    launch_init<T>(G, tables_, w, r, halo<T>(), partials_.get(), init_tiles_, s, op<T>());
    after_launch(s);
  }
  // red_b[1] = (z^0, r^0); red_b[0] = rho_B = (D^-1 B, B) when the residual rule starts from a w0, else 0
  launch_reduce(partials_.get(), init_tiles_.ntiles(), 2, stop_ref_data_ ? g_.h1h2 : 0.0, g_.h1h2, state_->red_b, state_, 0,
                reduce_ws_, s);
  after_launch(s);
  if (ca_) {  // set 0: z^0 = D^-1 r^0 (in r's buffer), p^0 = z^0; block counter 0
    std::memset(&ca_init_, 0, sizeof(CaState));
    ca_init_.s = ca_tiles_.s;  // (checked by load_checkpoint)
    HIP_CHECK(hipMemcpyAsync(ca_state_.get(), &ca_init_, sizeof(CaState), hipMemcpyHostToDevice, s));
    ca_blk_ = 0;
    ca_primed_ = false;
    launch_ca_init<T>(ca_geom_, ca_tables_, F.r, F.p0, s);
    after_launch(s);
  }
}

// pcg1: the radius-2 edges of the buffers the next sweep reads.  s-step 2-D blocks (no direct rows): the gh
// edge lines and corners of the set ca_halo_msgs would name (the set the next block reads, CaState::blk & 1
// mirrored by ca_blk_).  Both through the arena slots.
void GpuSubdomainSolver::halo_launch(hipStream_t s, bool unpack) {
  with_storage([&](auto t) {
    using T = decltype(t);
    const Fields<T> F = fields<T>();
    if (ca_)
      launch_ca_halo<T>(geom_, (ca_blk_ & 1) ? F.r2 : F.r, (ca_blk_ & 1) ? F.p1 : F.p0, halo<T>(), plan_.gh, unpack, s,
                        progress_dev_);
    else
      launch_pcg1_halo<T>(geom_, F.r, F.r2, F.p0, F.p1, halo<T>(), halo_target_, unpack, s, progress_dev_);
  });
  after_launch(s);
}

void GpuSubdomainSolver::set_direct_rows(bool on) {
  PMX_CHECK(!on || can_direct_rows(), "direct-row ghost exchange needs pcg1 on a row strip (x neighbours only)");
  direct_rows_ = on;
}

// Direct rows: `nrows` rows starting at local row srow of field f go to the neighbour across `slot`, whose
// rows land at rrow, as ONE span: the first nrows - 1 rows whole (a row's padding ends with column -1 of the
// next) and the last row's columns 0 .. ny+1; on a row strip the ghost columns are Dirichlet zeros
HaloMsg GpuSubdomainSolver::row_msg(int slot, int order, int f, int nrows, int64_t srow, int64_t rrow) const {
  return HaloMsg{slot, order, layout_.peer[slot], int((nrows - 1) * plan_.pitch + sd_.ny + 2),
                 field_ptr(f, srow), field_ptr(f, rrow)};
}

HaloMsgs GpuSubdomainSolver::halo_msgs() const {
  HaloMsgs out;
  if (!direct_rows_) {  // the packed slot buffers of the comm arena
    for (int slot = 0; slot < kHaloSlots; ++slot)
      if (layout_.active(slot))
        out.m[out.n++] = HaloMsg{slot, 0, layout_.peer[slot], layout_.edge_len[slot], send_dev(slot), recv_dev(slot)};
    return out;
  }
  if (ca_) return ca_halo_msgs(int(ca_blk_ & 1));
  // sweep t reads r^{t-1} from (t & 1 ? r2 : r) and p^{t-1} from (t & 1 ? p0 : p1) (k_pcg1)
  const bool odd = halo_target_ & 1;
  for (int slot = 0; slot < 2; ++slot) {
    if (layout_.peer[slot] < 0) continue;
    const int64_t srow = slot == 0 ? 1 : sd_.nx - 1, rrow = slot == 0 ? -1 : sd_.nx + 1;
    out.m[out.n++] = row_msg(slot, 0, odd ? 4 : 1, 2, srow, rrow);
    out.m[out.n++] = row_msg(slot, 1, odd ? 2 : 3, 2, srow, rrow);
  }
  return out;
}

void GpuSubdomainSolver::enqueue_halo_pack(hipStream_t s) {
  if ((pcg1_ || ca_) && geom_.nb != 0 && !direct_rows_) halo_launch(s, false);
}

void GpuSubdomainSolver::enqueue_halo_unpack(hipStream_t s) {
  if ((pcg1_ || ca_) && geom_.nb != 0 && !direct_rows_) halo_launch(s, true);
}

template <typename T>
void GpuSubdomainSolver::kernel_a(hipStream_t s, int part) {
  const Fields<T> F = fields<T>();
  if constexpr (sizeof(T) == 8) {
    if (block1_) {
      PMX_CHECK(part == 0, "block tiles run whole sweeps (undecomposed grids)");
      // the reduce_n ticket (never in flight together with this sweep: same stream)
      unsigned* ticket = block_fused_ ? reinterpret_cast<unsigned*>(reduce_ws_ + kReduceNOffset + 8 * kReduceMaxBlocks)
                                      : nullptr;
      launch_pcg1_block<T>(geom_, tables_, F.w, F.r, F.r2, F.p0, F.p1, partials_.get(), state_,
                           tiles1_for(w_sweep_next()), s, w_sweep_next(), weights1().v, ticket, progress_dev_);
      return;
    }
  }
  if (pcg1_)
    launch_pcg1<T>(geom_, tables_, F.w, F.r, F.r2, F.p0, F.p1, partials_.get(), state_, tiles1_for(w_sweep_next()), s,
                   part, w_sweep_next(), op<T>());
  else
    launch_pcg_a_wave<T>(geom_, tables_, F.r, F.p0, F.p1, halo<T>(), partials_.get(), state_, tiles_, opt_.exact, s);
}

template <typename T>
void GpuSubdomainSolver::kernel_b(hipStream_t s, bool pack) {
  if (pcg1_) return;  // the single sweep ran in phase a
  // pcg_b reads G.nb only to pack the send buffers: clearing it skips the packing
  DevGeom G = geom_;
  if (!pack) G.nb = 0;
  const Fields<T> F = fields<T>();
  launch_pcg_b_wave<T>(G, tables_, F.w, F.r, F.p0, F.p1, halo<T>(), partials_.get(), state_, tiles_b_, opt_.exact, s);
}

void GpuSubdomainSolver::enqueue_init(hipStream_t s) {
  HIP_CHECK(hipSetDevice(opt_.device));
  with_storage([&](auto t) { init_impl<decltype(t)>(s); });
}
void GpuSubdomainSolver::enqueue_stop_init(hipStream_t s) {
  if (spec_.stop != StopRule::kResidual) return;
  HIP_CHECK(hipSetDevice(opt_.device));
  launch_stop_init(state_, s);
  after_launch(s);
}
void GpuSubdomainSolver::enqueue_phase_a(hipStream_t s) {
  enqueue_kernel_a(s);
  enqueue_reduce_a(s);
}
void GpuSubdomainSolver::enqueue_phase_b(hipStream_t s, bool pack) {
  enqueue_kernel_b(s, pack);
  enqueue_reduce_b(s);
}
void GpuSubdomainSolver::enqueue_kernel_a(hipStream_t s) {
  with_storage([&](auto t) { kernel_a<decltype(t)>(s); });
  after_launch(s);
}
void GpuSubdomainSolver::enqueue_kernel_a_part(hipStream_t s, int part) {
  PMX_CHECK(pcg1_, "interior/frame sweeps are a pcg1 feature");
  with_storage([&](auto t) { kernel_a<decltype(t)>(s, part); });
  after_launch(s);
}
void GpuSubdomainSolver::enqueue_reduce_a(hipStream_t s) {
  if (block1_ && block_fused_) {  // the sweep finished its own reduction
    ++host_k_;
    return;
  }
  if (pcg1_) {
    // the sweep just enqueued (host_k not bumped yet) wrote one partial per tile of its tiling
    launch_reduce_n(partials_.get(), tiles1_for(w_sweep_next()).ntiles(), 5, weights1().v, state_->red_c, state_,
                    kSkipIfDone | kBumpIter, reduce_ws_, s, progress_dev_);
    ++host_k_;  // mirrors the S->it bump (see host_k())
    after_launch(s);
    return;
  }
  launch_reduce(partials_.get(), tiles_.ntiles(), 1, g_.h1h2, 0.0, state_->red_a, state_, kSkipIfDone, reduce_ws_, s);
  after_launch(s);
}
void GpuSubdomainSolver::enqueue_kernel_b(hipStream_t s, bool pack) {
  with_storage([&](auto t) { kernel_b<decltype(t)>(s, pack); });
  after_launch(s);
}
void GpuSubdomainSolver::enqueue_reduce_b(hipStream_t s) {
  if (pcg1_) return;
  const double wdiff = spec_.norm == Norm::kWeighted ? g_.h1h2 : 1.0;
  launch_reduce(partials_.get(), tiles_b_.ntiles(), 2, wdiff, g_.h1h2, state_->red_b, state_,
                kSkipIfDone | kBumpIter, reduce_ws_, s);
  after_launch(s);
}

void GpuSubdomainSolver::enqueue_poison_recv(hipStream_t s) {
  if (direct_rows_) {  // the ghost rows the next exchange writes
    const HaloMsgs ms = halo_msgs();
    for (int q = 0; q < ms.n; ++q)
      HIP_CHECK(hipMemsetAsync(ms.m[q].recv, 0xFF, size_t(ms.m[q].count) * plan_.elem, s));
    return;
  }
  const size_t off = layout_.recv_off[0];
  HIP_CHECK(hipMemsetAsync(arena_ + off, 0xFF, layout_.bytes - off, s));  // all-ones = NaN
}

namespace {
struct CkptHeader {
  char magic[8];
  int32_t version, M, N, gi0, gj0, rank, elem, norm;
  int64_t nx, ny, pitch, field_bytes, arena_bytes, max_iter;
  double delta;
};
constexpr char kCkptMagic[8] = {'P', 'M', 'X', 'C', 'K', 'P', 'T', '1'};
}  // namespace

// The version names the iteration algorithm and layout: v3 pcg2 (4 fields with 2 ghost rows), v5 pcg1
// (+ its w-cycle state, r2 appended), v6 the s-step PCG (r2 = the second z buffer appended, then
// CaState).  A checkpoint is written between batches, where every algorithm's state is exact: for the
// s-step no block's stop test is pending and w holds every applied block.
int GpuSubdomainSolver::ckpt_version() const { return ca_ ? 7 : pcg1_ ? 5 : 3; }

void GpuSubdomainSolver::save_checkpoint(std::ostream& os, hipStream_t s) const {
  HIP_CHECK(hipSetDevice(opt_.device));
  HIP_CHECK(hipStreamSynchronize(s));
  CkptHeader h{};
  std::memcpy(h.magic, kCkptMagic, 8);
  h.version = ckpt_version();
  h.M = spec_.M; h.N = spec_.N; h.gi0 = sd_.gi0(); h.gj0 = sd_.gj0();
  h.rank = sd_.rank; h.elem = int32_t(plan_.elem); h.norm = int32_t(spec_.norm);
  h.nx = sd_.nx; h.ny = sd_.ny; h.pitch = geom_.pitch; h.field_bytes = int64_t(plan_.field_bytes);
  h.arena_bytes = int64_t(layout_.bytes); h.max_iter = spec_.effective_max_iter(); h.delta = spec_.delta;
  os.write(reinterpret_cast<const char*>(&h), sizeof(h));
  // file order: fields 0 .. 3, the arena, then field 4 (r2 / the second z buffer) where there is one
  const size_t fb = plan_.field_bytes;
  std::vector<char> buf(std::max(4 * fb, layout_.bytes));
  HIP_CHECK(hipMemcpy(buf.data(), field_raw(0), 4 * fb, hipMemcpyDeviceToHost));
  os.write(buf.data(), std::streamsize(4 * fb));
  HIP_CHECK(hipMemcpy(buf.data(), arena_, layout_.bytes, hipMemcpyDeviceToHost));
  os.write(buf.data(), std::streamsize(layout_.bytes));
  if (plan_.nfields == 5) {
    HIP_CHECK(hipMemcpy(buf.data(), field_raw(4), fb, hipMemcpyDeviceToHost));
    os.write(buf.data(), std::streamsize(fb));
  }
  if (ca_) {
    CaState c{};
    HIP_CHECK(hipMemcpy(&c, ca_state_.get(), sizeof(CaState), hipMemcpyDeviceToHost));
    PMX_CHECK(c.pend_n == 0 && c.nupd <= 0, "s-step checkpoint inside a batch (a block's stop test is pending)");
    os.write(reinterpret_cast<const char*>(&c), sizeof(c));
    // a carried fused schedule: the next block's Gram partials (so a resume continues bitwise)
    const int32_t primed = ca_primed_ ? 1 : 0;
    os.write(reinterpret_cast<const char*>(&primed), sizeof(primed));
    if (primed) {
      std::vector<double> part(ca_primed_doubles());
      HIP_CHECK(hipMemcpy(part.data(), partials_.get(), part.size() * sizeof(double), hipMemcpyDeviceToHost));
      os.write(reinterpret_cast<const char*>(part.data()), std::streamsize(part.size() * sizeof(double)));
    }
  }
  PMX_CHECK(os.good(), "checkpoint write failed");
}

void GpuSubdomainSolver::load_checkpoint(std::istream& is, hipStream_t s) {
  HIP_CHECK(hipSetDevice(opt_.device));
  CkptHeader h{};
  is.read(reinterpret_cast<char*>(&h), sizeof(h));
  PMX_CHECK(is.good() && std::memcmp(h.magic, kCkptMagic, 8) == 0 && h.version == ckpt_version(),
            "not a pmx checkpoint of this iteration algorithm and layout (v3 pcg2, v5 pcg1, v7 s-step; file v"
                << h.version << ", solver v" << ckpt_version() << ")");
  PMX_CHECK(h.M == spec_.M && h.N == spec_.N && h.gi0 == sd_.gi0() && h.gj0 == sd_.gj0() &&
                h.nx == sd_.nx && h.ny == sd_.ny && h.rank == sd_.rank,
            "checkpoint is for a different grid/decomposition (M=" << h.M << " N=" << h.N << " rank "
                                                                  << h.rank << ")");
  const size_t fb = plan_.field_bytes;
  PMX_CHECK(h.elem == int32_t(plan_.elem) && h.pitch == geom_.pitch && h.field_bytes == int64_t(fb) &&
                h.arena_bytes == int64_t(layout_.bytes),
            "checkpoint precision/layout differs from this solver");
  PMX_CHECK(h.norm == int32_t(spec_.norm) && h.delta == spec_.delta &&
                h.max_iter == spec_.effective_max_iter(),
            "checkpoint was written with a different stop rule (norm/delta/max_iter)");
  std::vector<char> buf(std::max(4 * fb, layout_.bytes));
  is.read(buf.data(), std::streamsize(4 * fb));
  PMX_CHECK(is.good(), "truncated checkpoint (fields)");
  HIP_CHECK(hipStreamSynchronize(s));
  HIP_CHECK(hipMemcpy(field_raw(0), buf.data(), 4 * fb, hipMemcpyHostToDevice));
  is.read(buf.data(), std::streamsize(layout_.bytes));
  PMX_CHECK(is.good(), "truncated checkpoint (scalars/halos)");
  PcgState ck{};
  std::memcpy(&ck, buf.data() + layout_.state_off, sizeof(PcgState));
  // the state carries its stop rule (files of builds without one hold zeros: the step rule)
  const bool same_rule = ck.stop == int(spec_.stop) &&
                         (spec_.stop == StopRule::kStep || (ck.rtol == spec_.rtol && ck.atol == spec_.atol));
  if (!same_rule) {
    auto show = [](int rule, double rtol, double atol) {
      std::ostringstream o;
      o << "stop=" << stop_rule_name(StopRule(rule));
      if (rule == int(StopRule::kResidual)) o << " rtol=" << rtol << " atol=" << atol;
      return o.str();
    };
    PMX_CHECK(false, "checkpoint was written with " << show(ck.stop, ck.rtol, ck.atol) << ", this session runs "
                                                      << show(int(spec_.stop), spec_.rtol, spec_.atol));
  }
  HIP_CHECK(hipMemcpy(arena_, buf.data(), layout_.bytes, hipMemcpyHostToDevice));
  host_k_ = ck.it;
  if (plan_.nfields == 5) {
    is.read(buf.data(), std::streamsize(fb));
    PMX_CHECK(is.good(), "truncated checkpoint (r2 / second z buffer)");
    HIP_CHECK(hipMemcpy(field_raw(4), buf.data(), fb, hipMemcpyHostToDevice));
  }
  if (ca_) {
    CaState c{};
    is.read(reinterpret_cast<char*>(&c), sizeof(c));
    PMX_CHECK(is.good(), "truncated checkpoint (s-step state)");
    PMX_CHECK(c.s == ca_tiles_.s, "checkpoint was written with s = " << c.s << ", this solver runs s = " << ca_tiles_.s);
    c.ticket = 0u;
    HIP_CHECK(hipMemcpy(ca_state_.get(), &c, sizeof(CaState), hipMemcpyHostToDevice));
    ca_blk_ = c.blk;  // the (z, p) set the next block reads
    int32_t primed = 0;
    is.read(reinterpret_cast<char*>(&primed), sizeof(primed));
    PMX_CHECK(is.good() && (primed == 0 || (primed == 1 && ca_fused())), "checkpoint: bad s-step schedule flag");
    if (primed) {
      std::vector<double> part(ca_primed_doubles());
      is.read(reinterpret_cast<char*>(part.data()), std::streamsize(part.size() * sizeof(double)));
      PMX_CHECK(is.good(), "truncated checkpoint (carried Gram partials)");
      HIP_CHECK(hipMemcpy(partials_.get(), part.data(), part.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    ca_primed_ = primed != 0;
  }
}

void GpuSubdomainSolver::enqueue_pack(hipStream_t s) {
  if (geom_.nb == 0 || pcg1_) return;
  with_storage([&](auto t) {
    using T = decltype(t);
    const Fields<T> F = fields<T>();
    launch_edge_r<T>(geom_, tables_, F.r, F.p0, F.p1, halo<T>(), state_, opt_.exact, s);
  });
  after_launch(s);
}

double GpuSubdomainSolver::bench_kernel(int which, int abl, int reps, hipStream_t s) {
  PMX_CHECK(!ca_, "not available for the s-step solver");
  HIP_CHECK(hipSetDevice(opt_.device));
  PcgState& st = host_state_.get()[1];
  std::memset(&st, 0, sizeof(st));
  st.delta = 0.0;
  // a mid-solve iteration: beta path, p^{k-1} read.  which = 2: pcg_b on an odd iteration (w
  // step deferred, see k_pcg_b_rows); which = 1 is the even (paired w update) one
  st.it = which == 2 ? 3 : 2;
  st.max_iter = int64_t(1) << 40;
  st.norm = int(spec_.norm);
  st.red_a[0] = 1.0;
  st.red_b[0] = 1.0;
  st.red_b[1] = 1e-3;
  st.zr[0] = st.zr[1] = 1e-3;
  st.alpha[0] = st.alpha[1] = 1.0;
  for (int q = 0; q < 4; ++q) st.alpha1[q] = st.beta1[q] = 1.0;
  st.w_cycle = w_cycle();
  host_k_ = st.it;
  st.red_c[0] = 1e-3;
  st.red_c[1] = st.red_c[3] = st.red_c[4] = 1.0;
  st.pair_w = opt_.pair_w ? 1 : 0;
  st.pair_min_beta = opt_.pair_w == 2 ? HUGE_VAL : 1e-3;
  const TileCfg saved = tiles_, saved_b = tiles_b_;
  tiles_.abl = abl;
  tiles_b_.abl = abl;
  auto launch = [&] {
    with_storage([&](auto t) {
      using T = decltype(t);
      if (which == 0 || pcg1_) kernel_a<T>(s); else kernel_b<T>(s);
    });
  };
  for (int k = 0; k < 2; ++k) {
    HIP_CHECK(hipMemcpyAsync(state_, &st, sizeof(PcgState), hipMemcpyHostToDevice, s));
    launch();
  }
  HIP_CHECK(hipStreamSynchronize(s));
  const Event e0 = make_event(), e1 = make_event();
  float total = 0.f;
  for (int k = 0; k < reps; ++k) {
    HIP_CHECK(hipMemcpyAsync(state_, &st, sizeof(PcgState), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipEventRecord(e0.get(), s));
    launch();
    HIP_CHECK(hipEventRecord(e1.get(), s));
    HIP_CHECK(hipEventSynchronize(e1.get()));
    float ms = 0.f;
    HIP_CHECK(hipEventElapsedTime(&ms, e0.get(), e1.get()));
    total += ms;
  }
  tiles_ = saved;
  tiles_b_ = saved_b;
  return double(total) / reps;
}

PcgState GpuSubdomainSolver::read_state(hipStream_t s) const {
  HIP_CHECK(hipSetDevice(opt_.device));
  HIP_CHECK(hipMemcpyAsync(host_state_.get(), state_, sizeof(PcgState), hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  return *host_state_;
}

std::vector<double> GpuSubdomainSolver::read_partials(hipStream_t s) const {
  HIP_CHECK(hipSetDevice(opt_.device));
  std::vector<double> h(npart_ * 5);
  HIP_CHECK(hipMemcpyAsync(h.data(), partials_.get(), h.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  return h;
}

std::vector<double> GpuSubdomainSolver::download_field(int which, hipStream_t s) const {
  HIP_CHECK(hipSetDevice(opt_.device));
  const size_t n = size_t(sd_.nx + 2) * geom_.pitch;
  std::vector<char> raw(n * plan_.elem);
  HIP_CHECK(hipMemcpyAsync(raw.data(), field_base(which), raw.size(), hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  std::vector<double> out(size_t(sd_.nx + 2) * (sd_.ny + 2));
  for (int li = 0; li <= sd_.nx + 1; ++li)
    for (int lj = 0; lj <= sd_.ny + 1; ++lj) {
      const size_t src = size_t(li) * geom_.pitch + lj;
      out[size_t(li) * (sd_.ny + 2) + lj] =
          plan_.elem == 8 ? reinterpret_cast<const double*>(raw.data())[src]
                     : double(reinterpret_cast<const float*>(raw.data())[src]);
    }
  return out;
}

std::vector<double> GpuSubdomainSolver::download_w(hipStream_t s) const {
  const std::vector<double> f = download_field(0, s);
  // the pending w steps (pending_w), applied here and rounded to the storage type like a device update
  const PendingW pw = pending_w(read_state(s));
  std::vector<double> pk[2];
  for (int q = 0; q < pw.n; ++q) pk[q] = download_field(pw.field[q], s);
  std::vector<double> out(size_t(sd_.nx) * sd_.ny);
  for (int li = 1; li <= sd_.nx; ++li)
    for (int lj = 1; lj <= sd_.ny; ++lj) {
      const size_t src = size_t(li) * (sd_.ny + 2) + lj;
      double v = f[src];
      for (int q = 0; q < pw.n; ++q) v = std::fma(pw.a[q], pk[q][src], v);
      if (pw.n && plan_.elem == 4) v = double(float(v));
      out[size_t(li - 1) * sd_.ny + (lj - 1)] = v;
    }
  return out;
}

void GpuSubdomainSolver::gather_w_device(double* out, int64_t ld, hipStream_t s) const {
  HIP_CHECK(hipSetDevice(opt_.device));
  PMX_CHECK(out && ld >= spec_.N + 1, "gather_w_device needs an (M+1) x (N+1) array with row stride >= N+1");
  const PendingW pw = pending_w(read_state(s));
  // the owned nodes, widened by the global boundary row / column where the block touches it
  const int li0 = sd_.gi0() == 0 ? 0 : 1, li1 = sd_.gi0() + sd_.nx + 1 == spec_.M ? sd_.nx + 1 : sd_.nx;
  const int lj0 = sd_.gj0() == 0 ? 0 : 1, lj1 = sd_.gj0() + sd_.ny + 1 == spec_.N ? sd_.ny + 1 : sd_.ny;
  with_storage([&](auto t) {
    using T = decltype(t);
    launch_gather<T>(fields<T>().w, pending_p<T>(pw, 0), pw.a[0], pending_p<T>(pw, 1), pw.a[1], pw.n, geom_.pitch, out,
                     ld, li0, lj0, li1 - li0 + 1, lj1 - lj0 + 1, sd_.gi0(), sd_.gj0(), spec_.M, spec_.N, s);
  });
  after_launch(s);
}

}  // namespace pmx
