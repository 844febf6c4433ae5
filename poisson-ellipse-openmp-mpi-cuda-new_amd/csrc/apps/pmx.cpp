// pmx — command-line front end (component X6/X7 of SURVEY §2.6, CLI of §5.6).
//
// Backward compatible with the reference programs: `pmx M N` mirrors stages 2-4
// (stage4-mpi+cuda/poisson_mpi_cuda_f.cu:996-1000), defaults reproduce the reference problem
// (ellipse x^2+4y^2<1, delta=1e-6, max_iter=(M-1)(N-1), weighted norm).  The superset:
//
//   pmx [M N] [--ax 1.0 --by 0.5] [--box -1,1,-0.6,0.6] [--f 1.0] [--delta 1e-6] [--max-iter K]
//       [--breakdown-tol 1e-15] [--sigma 0] [--stop step|residual --rtol 1e-8 --atol 0]
//       [--backend cpu|omp|hip] [--threads T] [--ranks P] [--gpus G] [--comm self|local|rccl]
//       [--split reference|auto|rows|cols] [--dtype fp64|fp32|mixed] [--norm weighted|unweighted]
//       [--exact] [--graph-batch 32] [--tile-rows 0] [--kernel wave] [--vec 2] [--waves 4]
//       [--block 256] [--device D] [--vec-b V] [--waves-b W] [--tile-rows-b R] [--b-kernel rows|ring]
//       [--dump sol.txt] [--dump-stride s] [--json] [--banner stage0..stage4]
//       [--profile-phases N] [--check] [--overlap on|off] [--poison-halos]
//       [--checkpoint FILE [--checkpoint-every K]] [--resume FILE]
//       [--sweep-grids 10x10,20x20,40x40] [--sweep-threads 2,4,8,16] [--plan] [--placement K]
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <iomanip>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "pmx/common.hpp"
#include "pmx/cpu_pcg.hpp"
#include "pmx/report.hpp"
#include "pmx/session.hpp"

using namespace pmx;

namespace {

struct Cli {
  ProblemSpec spec;
  std::string backend = "auto", comm = "auto", banner = "auto", dump, split = "reference";
  std::string checkpoint, resume;
  int64_t checkpoint_every = 0;
  // benchmark sweeps (the reference's hard-coded drivers): grids for any backend,
  // OpenMP thread counts for cpu/omp (stage0/Withoutopenmp1.cpp:177, stage1-openmp/*:214)
  std::vector<std::pair<int, int>> sweep_grids;
  std::vector<int> sweep_threads;
  int threads = 1, ranks = 1, gpus = 0, dump_stride = 1, device = 0;
  int64_t profile = 0;
  bool json = false, plan = false;
  GpuOptions opt;
};

[[noreturn]] void usage(const char* msg) {
  if (msg) std::cerr << "pmx: " << msg << "\n";
  std::cerr << "usage: pmx [M N] [--ax A] [--by B] [--box a1,b1,a2,b2] [--f F] [--delta D] [--max-iter K]\n"
               "           [--breakdown-tol T] [--sigma S] [--stop step|residual] [--rtol R] [--atol A]\n"
               "           [--backend cpu|omp|hip] [--threads T] [--ranks P] [--gpus G]\n"
               "           [--comm self|local|rccl] [--split reference|auto|rows|cols]\n"
               "           [--dtype fp64|fp32|mixed] [--norm weighted|unweighted] [--exact]\n"
               "           [--graph-batch N] [--tile-rows R] [--kernel wave] [--vec V]\n"
               "           [--waves W] [--block B] [--device D] [--vec-b V] [--waves-b W] [--tile-rows-b R]\n"
               "           [--b-kernel rows|ring] [--pair-w 0|1|2]\n"
               "           [--dump FILE] [--dump-stride S] [--json] [--banner stage0..stage4]\n"
               "           [--profile-phases N] [--check] [--overlap on|off] [--poison-halos]\n"
               "           [--checkpoint FILE [--checkpoint-every K]] [--resume FILE]\n"
               "           [--sweep-grids MxN,MxN,...] [--sweep-threads T,T,...] [--plan] [--placement K]\n"
               "           [--algo auto|pcg1|pcg2|ca] [--ca-s 2|3]\n";
  std::exit(msg ? 2 : 0);
}

Split parse_split(const std::string& s) {
  if (s == "reference") return Split::kReference;
  if (s == "auto") return Split::kAuto;
  if (s == "rows") return Split::kRows;
  if (s == "cols") return Split::kCols;
  usage("bad --split");
}

Cli parse(int argc, char** argv) {
  Cli c;
  std::vector<std::string> pos;
  for (int i = 1; i < argc; ++i) {
    std::string a = argv[i];
    auto val = [&]() -> std::string {
      if (i + 1 >= argc) usage(("missing value for " + a).c_str());
      return argv[++i];
    };
    if (a == "-h" || a == "--help") usage(nullptr);
    else if (a == "--ax") c.spec.ax = std::atof(val().c_str());
    else if (a == "--by") c.spec.by = std::atof(val().c_str());
    else if (a == "--f") c.spec.F = std::atof(val().c_str());
    else if (a == "--delta") c.spec.delta = std::atof(val().c_str());
    else if (a == "--breakdown-tol") c.spec.breakdown_tol = std::atof(val().c_str());
    else if (a == "--max-iter") c.spec.max_iter = std::atoll(val().c_str());
    else if (a == "--sigma") c.spec.sigma = std::atof(val().c_str());  // (-Δ + sigma) u = f, sigma >= 0
    else if (a == "--stop") {
      const std::string v = val();
      if (v != "step" && v != "residual") usage("--stop step|residual");
      c.spec.stop = v == "residual" ? StopRule::kResidual : StopRule::kStep;
    }
    else if (a == "--rtol") c.spec.rtol = std::atof(val().c_str());
    else if (a == "--atol") c.spec.atol = std::atof(val().c_str());
    else if (a == "--box") {
      const std::string v = val();
      if (std::sscanf(v.c_str(), "%lf,%lf,%lf,%lf", &c.spec.A1, &c.spec.B1, &c.spec.A2, &c.spec.B2) != 4)
        usage("--box needs a1,b1,a2,b2");
    } else if (a == "--backend") c.backend = val();
    else if (a == "--threads") c.threads = std::atoi(val().c_str());
    else if (a == "--ranks") c.ranks = std::atoi(val().c_str());
    else if (a == "--gpus") c.gpus = std::atoi(val().c_str());
    else if (a == "--comm") c.comm = val();
    else if (a == "--split") c.split = val();
    else if (a == "--dtype") {
      const std::string v = val();
      // fp32: fields and the single-pass sweep's stencil arithmetic in fp32; mixed: fp32 fields,
      // every stencil/update in fp64 registers.  Both keep reductions and PCG scalars in fp64.
      if (v != "fp64" && v != "fp32" && v != "mixed") usage("--dtype fp64|fp32|mixed");
      c.opt.dtype = v == "fp64" ? DType::kFp64 : DType::kFp32;
      c.opt.arith32 = v == "fp32" ? 1 : 0;
    } else if (a == "--norm") {
      const std::string v = val();
      if (v != "weighted" && v != "unweighted") usage("--norm weighted|unweighted");
      c.spec.norm = v == "weighted" ? Norm::kWeighted : Norm::kUnweighted;
    } else if (a == "--exact") c.opt.exact = true;
    else if (a == "--graph-batch") c.opt.graph_batch = std::atoi(val().c_str());
    else if (a == "--tile-rows") c.opt.tile_rows = std::atoi(val().c_str());
    else if (a == "--block") (void)val();  // accepted for compatibility: the wave tiles have no such width
    else if (a == "--vec") c.opt.vec = std::atoi(val().c_str());
    else if (a == "--waves") c.opt.waves = std::atoi(val().c_str());
    else if (a == "--vec-b") c.opt.vec_b = std::atoi(val().c_str());
    else if (a == "--waves-b") c.opt.waves_b = std::atoi(val().c_str());
    else if (a == "--tile-rows-b") c.opt.tile_rows_b = std::atoi(val().c_str());
    else if (a == "--b-kernel") {
      const std::string v = val();
      if (v != "rows" && v != "ring") usage("--b-kernel rows|ring");
      c.opt.b_ring = v == "ring";
    }
    else if (a == "--pair-w") c.opt.pair_w = std::atoi(val().c_str());
    else if (a == "--kernel") {
      const std::string v = val();
      if (v != "wave") usage("--kernel wave (the round-1 lds kernels are retired)");
    }
    else if (a == "--device") c.device = std::atoi(val().c_str());
    else if (a == "--dump") c.dump = val();
    else if (a == "--dump-stride") c.dump_stride = std::atoi(val().c_str());
    else if (a == "--json") c.json = true;
    else if (a == "--banner") c.banner = val();
    else if (a == "--profile-phases") c.profile = std::atoll(val().c_str());
    else if (a == "--check") c.opt.check = true;
    else if (a == "--poison-halos") c.opt.poison_halos = true;
    else if (a == "--plan") c.plan = true;
    else if (a == "--placement") c.opt.placement = std::atoi(val().c_str());  // probe K field blocks
    else if (a == "--algo") {
      // auto: the s-step PCG on big fp64 grids / row strips when its fields fit, else pcg1 / pcg2
      // (choose_algo); pcg1 = single pass, pcg2 = two sweeps, ca = the s-step PCG (ca_kernels.hip)
      const std::string v = val();
      if (v == "auto") c.opt.algo = -1;
      else if (v == "pcg1") c.opt.algo = 1;
      else if (v == "pcg2") c.opt.algo = 2;
      else if (v == "ca") c.opt.algo = 3;
      else usage("--algo auto|pcg1|pcg2|ca");
    } else if (a == "--ca-s") {
      c.opt.ca_s = std::atoi(val().c_str());
      if (c.opt.ca_s != 2 && c.opt.ca_s != 3) usage("--ca-s 2|3");
    }
    else if (a == "--sweep-grids") {
      std::string v = val() + ",";
      for (size_t p = 0, q; (q = v.find(',', p)) != std::string::npos; p = q + 1) {
        const std::string g = v.substr(p, q - p);
        const size_t x = g.find('x');
        if (g.empty()) continue;
        if (x == std::string::npos) usage("--sweep-grids MxN,MxN,...");
        c.sweep_grids.emplace_back(std::atoi(g.substr(0, x).c_str()), std::atoi(g.substr(x + 1).c_str()));
      }
    } else if (a == "--sweep-threads") {
      std::string v = val() + ",";
      for (size_t p = 0, q; (q = v.find(',', p)) != std::string::npos; p = q + 1)
        if (q > p) c.sweep_threads.push_back(std::atoi(v.substr(p, q - p).c_str()));
    }
    else if (a == "--checkpoint") c.checkpoint = val();
    else if (a == "--checkpoint-every") c.checkpoint_every = std::atoll(val().c_str());
    else if (a == "--resume") c.resume = val();
    else if (a == "--overlap") {
      const std::string v = val();
      if (v != "on" && v != "off") usage("--overlap on|off");
      c.opt.overlap = v == "on";
    }
    else if (!a.empty() && a[0] == '-') usage(("unknown option " + a).c_str());
    else pos.push_back(a);
  }
  if (pos.size() == 2) {
    c.spec.M = std::atoi(pos[0].c_str());
    c.spec.N = std::atoi(pos[1].c_str());
  } else if (!pos.empty()) {
    usage("expected positional M N");
  }
  if (c.backend == "auto") {
    int n = 0;
    c.backend = (hipGetDeviceCount(&n) == hipSuccess && n > 0) ? "hip" : (c.threads > 1 ? "omp" : "cpu");
    (void)hipGetLastError();
  }
  if (c.banner == "auto") {
    if (c.backend == "hip") c.banner = "stage4";
    else if (c.ranks > 1) c.banner = c.threads > 1 ? "stage3" : "stage2";
    else c.banner = c.spec.norm == Norm::kUnweighted ? "stage0" : "stage1";
  }
  c.opt.device = c.device;
  return c;
}

double now() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

int run_cpu(Cli& c, double t_prog, bool header = true, bool footer = true) {
  const ProblemSpec& s = c.spec;
  const bool stage0 = c.banner == "stage0";
  if (c.banner == "stage1" && header)
    std::cout << "--- (Variant 9: Ellipse x^2 + 4y^2 < 1, OpenMP Test) ---\nGrid: M=" << s.M << ", N=" << s.N
              << "\n--------------------------------------------------------\n";
  if (c.banner == "stage2" && header)
    std::cout << "Pure MPI 2D run with " << c.ranks << " processes; M=" << s.M << ", N=" << s.N << std::endl;
  if (c.banner == "stage3" && header)
    std::cout << "MPI/OpenMP run with " << c.ranks << " MPI processes; M=" << s.M << ", N=" << s.N << std::endl;
  const int threads = c.backend == "cpu" ? 1 : c.threads;
  SolveResult r = c.ranks > 1 ? cpu_solve_decomposed(s, c.ranks, parse_split(c.split), threads, true)
                              : cpu_solve(s, threads, true);
  if (r.status == Status::kConverged) print_converged(r.iters, s, stage0 || c.banner == "stage1");
  if (c.banner == "stage1") {
    std::cout << "Threads = " << std::setw(2) << threads << " | Time = " << std::fixed << std::setprecision(3)
              << r.seconds << " s\n";
    if (footer) std::cout << "--------------------------------------------------------\n";
  } else {
    std::cout << "M=" << s.M << ", N=" << s.N << " | Iter=" << r.iters << " | Time=" << std::fixed
              << std::setprecision(stage0 ? 4 : 6) << r.seconds << " s\n";
  }
  const ErrorNorms e = error_norms(s, r.w);
  if (!c.dump.empty()) write_ascii(c.dump, s, r.w, c.dump_stride, r.iters);
  if (c.json) {
    JsonLine j;
    j.ks("backend", c.backend).kv("M", s.M).kv("N", s.N).kv("ranks", c.ranks).kv("threads", threads)
        .kv("iters", r.iters).ks("status", status_name(r.status)).kv("seconds", r.seconds)
        .kv("mlups", double(s.M - 1) * (s.N - 1) * r.iters / r.seconds / 1e6);
    // the closed-form solution the errors compare with holds for sigma = 0 only
    if (s.sigma == 0.0) j.kv("l2_error", e.l2).kv("max_error", e.max_err);
    j.kv("max_w", e.max_w).kv("sigma", s.sigma);
    if (s.stop == StopRule::kResidual)
      j.ks("stop", "residual").kv("rtol", s.rtol).kv("atol", s.atol).kv("residual", r.residual)
          .kv("residual_ref", r.residual_ref);
    j.kv("total_seconds", now() - t_prog);
    std::cout << j.str() << std::endl;
  }
  return 0;
}

// --plan: decomposition and device-memory plan for the requested run, no solve (SURVEY §5.7:
// subgrids sized against the HBM of each MI355X)
int run_plan(const Cli& c) {
  const ProblemSpec& s = c.spec;
  const int ranks = std::max({1, c.gpus, c.ranks});
  const ProcGrid pg = make_process_grid(ranks, s.M, s.N, parse_split(c.split));
  double dev_bytes = 288e9;  // MI355X HBM3E when no device is visible
  std::string dev_src = "assumed 288 GB (no device visible)";
  int n = 0;
  if (hipGetDeviceCount(&n) == hipSuccess && n > 0) {
    size_t fb = 0, tb = 0;
    if (hipSetDevice(c.device) == hipSuccess && hipMemGetInfo(&fb, &tb) == hipSuccess) {
      dev_bytes = double(tb);
      std::ostringstream o;
      o << "device " << c.device << ": " << tb / 1e9 << " GB total, " << fb / 1e9 << " GB free";
      dev_src = o.str();
    }
  }
  (void)hipGetLastError();
  const int gpus = std::max(1, c.gpus);
  std::cout << "plan: M=" << s.M << ", N=" << s.N << ", " << ranks << " subdomain(s) as " << pg.Px << " x "
            << pg.Py << ", dtype " << dtype_name(c.opt) << "\n"
            << "memory: " << dev_src << "\n";
  const int subs_per_device = c.gpus > 1 ? 1 : ranks;  // LocalComm: every subdomain on one device
  const int algo = choose_algo(s, pg, resolve_options(c.opt), dev_bytes, subs_per_device, true);
  std::cout << "iteration: "
            << (algo == 3   ? "s-step PCG (ca, s = " + std::to_string(c.opt.ca_s) + ": 5 fields + 2 face fields)"
                : algo == 1 ? std::string("pcg1 (single pass, 5 fields)")
                            : std::string("pcg2 (two sweeps, 4 fields)"))
            << "\n";
  size_t worst = 0;
  for (int r = 0; r < ranks; ++r) {
    const Subdomain sd = decompose_2d(s.M, s.N, pg, r);
    const size_t b = GpuSubdomainSolver::estimate_device_bytes_algo(s, sd, c.opt.dtype, algo);
    worst = std::max(worst, b);
    std::cout << "  rank " << r << ": " << sd.nx << " x " << sd.ny << " nodes, ~" << b / 1e9 << " GB\n";
  }
  // subdomains on one device add up (LocalComm); one per device otherwise
  const size_t per_device = c.gpus > 1 ? worst : worst * size_t(ranks);
  std::cout << "per device: ~" << per_device / 1e9 << " GB -> "
            << (double(per_device) <= dev_bytes ? "fits" : "DOES NOT FIT") << "\n"
            << "largest square grid on " << gpus << " such device(s): ~"
            << max_square_grid(dev_bytes, gpus, c.opt.dtype, 0.1, -1) << "^2 (pcg1)";
  if (c.opt.dtype == DType::kFp64)
    std::cout << ", ~" << max_square_grid(dev_bytes, gpus, c.opt.dtype, 0.1, 3) << "^2 with the s-step PCG";
  std::cout << "\n";
  return double(per_device) <= dev_bytes ? 0 : 4;
}

int run_hip(Cli& c, double t_prog) {
  SessionConfig cfg;
  cfg.spec = c.spec;
  cfg.opt = c.opt;
  cfg.split = parse_split(c.split);
  const int gpus = std::max(1, c.gpus);
  if (c.gpus > 1) {
    cfg.world = gpus;
    cfg.comm = CommKind::kRccl;
    for (int r = 0; r < gpus; ++r) { cfg.ranks.push_back(r); cfg.devices.push_back(c.device + r); }
    cfg.rccl_uid = rccl_unique_id();
  } else {
    cfg.world = c.ranks;
    cfg.comm = c.ranks > 1 ? CommKind::kLocal : CommKind::kSelf;
  }
  if (c.comm == "rccl" && c.gpus <= 1) PMX_CHECK(false, "--comm rccl needs --gpus > 1");
  const ProblemSpec& s = c.spec;
  std::cout << "MPI + CUDA 2D run with " << cfg.world << " processes; M=" << s.M << ", N=" << s.N << std::endl;
  const double t_before = now();
  Session sess(cfg);
  RunStats st;
  if (!c.resume.empty() || !c.checkpoint.empty()) {
    // periodic checkpoints go to --checkpoint (default: the --resume file)
    const std::string out = c.checkpoint.empty() ? c.resume : c.checkpoint;
    st = sess.solve_checkpointed(out, c.checkpoint_every, c.resume);
  } else {
    st = sess.solve();
  }
  if (!c.checkpoint.empty()) sess.save_checkpoint(c.checkpoint);  // final state
  const double t_after = now();
  if (st.status == Status::kConverged) print_converged(st.iters, s, false);
  std::vector<double> w;  // gathered before profiling, which restarts the solver
  if (!c.dump.empty() || c.json) w = sess.gather_local_w();
  RunStats ph;
  if (c.profile > 0) {
    sess.init();
    ph = sess.profile(c.profile);
    const double scale = double(st.iters) / double(c.profile);
    // the reference's 5 buckets (stage4-mpi+cuda/poisson_mpi_cuda_f.cu:970-979), scaled from the
    // profiled iterations to the whole solve; copy and precond are 0 by construction here
    std::cout << "   GPU compute time (Ap + D^{-1}r, max over ranks) ~ " << (ph.t_kernel_a + ph.t_kernel_b) * scale << " s\n"
              << "   Host<->Device copy time (max over ranks)        ~ " << 0.0 << " s\n"
              << "   MPI halo exchange time (max over ranks)         ~ " << ph.t_comm * scale << " s\n"
              << "   Preconditioner CPU part time (max over ranks)   ~ " << 0.0 << " s\n"
              << "   Dot products time (max over ranks)              ~ " << ph.t_reduce * scale << " s\n"
              << "   (buckets of the fused iteration: compute = the whole single sweep (A p, r/w update,\n"
              << "    D^{-1} r, A z); copy and preconditioner are 0 by construction -- no host staging, D^{-1}\n"
              << "    fused into the sweep; dot = the device reduction; MPI = all-reduce + ghost exchange)\n";
  }
  std::cout << "M=" << s.M << ", N=" << s.N << " | Iter=" << st.iters << " | Total Time=" << std::fixed
            << std::setprecision(6) << (t_after - t_prog) << " s\n"
            << "   Init time (program)      ~ " << (t_before - t_prog) + st.init_seconds << " s\n"
            << "   Solver time (MPI+CUDA)   ~ " << st.solve_seconds << " s\n"
            << "   Finalization time        ~ " << 0.0 << " s\n";
  if (!c.dump.empty()) write_ascii(c.dump, s, w, c.dump_stride, st.iters);
  if (c.json) {
    const ErrorNorms e = error_norms(s, w);
    JsonLine j;
    j.ks("backend", "hip").kv("M", s.M).kv("N", s.N).kv("ranks", cfg.world).ks("comm", sess.comm_name())
        .ks("dtype", dtype_name(c.opt)).ks("algo", sess.algo_name()).kv("iters", st.iters)
        .ks("status", status_name(st.status)).kv("solve_seconds", st.solve_seconds)
        .kv("init_seconds", st.init_seconds)
        .kv("mlups", double(s.M - 1) * (s.N - 1) * st.iters / st.solve_seconds / 1e6)
        .kv("us_per_iter", st.solve_seconds / std::max<int64_t>(1, st.iters) * 1e6);
    if (s.sigma == 0.0) j.kv("l2_error", e.l2).kv("max_error", e.max_err);  // (closed form: sigma = 0 only)
    j.kv("max_w", e.max_w).kv("sigma", s.sigma);
    if (s.stop == StopRule::kResidual)
      j.ks("stop", "residual").kv("rtol", s.rtol).kv("atol", s.atol).kv("residual", st.residual)
          .kv("residual_ref", st.residual_ref);
    j.kv("device_bytes", sess.device_bytes()).kv("total_seconds", now() - t_prog);
    if (c.profile > 0)
      j.kv("profiled_iters", c.profile).kv("phase_kernel_a_s", ph.t_kernel_a)
          .kv("phase_kernel_b_s", ph.t_kernel_b).kv("phase_reduce_s", ph.t_reduce)
          .kv("phase_allreduce_s", ph.t_allreduce).kv("phase_halo_s", ph.t_halo);
    std::cout << j.str() << std::endl;
  }
  return st.nan ? 3 : 0;
}

}  // namespace

int main(int argc, char** argv) {
  const double t_prog = now();
  try {
    Cli c = parse(argc, argv);
    c.spec.validate();
    if (c.backend != "cpu" && c.backend != "omp" && c.backend != "hip") usage("unknown --backend");
    if (c.plan) return run_plan(c);
    if (c.sweep_grids.empty() && c.sweep_threads.empty()) {
      return c.backend == "hip" ? run_hip(c, t_prog) : run_cpu(c, t_prog);
    }
    // sweep: grids outer, thread counts inner; header/footer once per grid like stage 1
    if (c.sweep_grids.empty()) c.sweep_grids.emplace_back(c.spec.M, c.spec.N);
    if (c.sweep_threads.empty()) c.sweep_threads.push_back(c.threads);
    int rc = 0;
    for (const auto& g : c.sweep_grids) {
      for (size_t k = 0; k < c.sweep_threads.size(); ++k) {
        Cli r = c;
        r.spec.M = g.first;
        r.spec.N = g.second;
        r.spec.validate();
        r.threads = c.sweep_threads[k];
        if (r.backend == "cpu" && r.threads > 1) r.backend = "omp";
        rc |= r.backend == "hip" ? run_hip(r, now())
                                 : run_cpu(r, now(), k == 0, k + 1 == c.sweep_threads.size());
      }
    }
    return rc;
  } catch (const std::exception& e) {
    std::cerr << e.what() << std::endl;
    return 1;
  }
}
