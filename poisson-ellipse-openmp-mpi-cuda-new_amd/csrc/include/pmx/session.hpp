// A solve session: decomposition + per-subdomain GPU solvers + comm backend + driver.
// Shared by the C++ CLI (apps/pmx.cpp) and the Python bindings.
#pragma once

#include <initializer_list>
#include <memory>
#include <string>
#include <vector>

#include "pmx/common.hpp"
#include "pmx/gpu_solver.hpp"

namespace pmx {

enum class CommKind : int { kSelf = 0, kLocal = 1, kRccl = 2, kIpc = 3, kLoopback = 4 };

// A global (M+1) x (N+1) fp64 field handed to a session: host memory, or memory of the session's
// device.  ld: the row stride in elements (0: dense, N + 1); the column stride is 1.
// A device field follows stream order without any synchronisation by the caller.  An input is read
// after the work enqueued on `stream` (its producer's) before the call: the session records an event
// there and its own streams wait for it.  An output is complete for work enqueued on `stream` after
// the call: `stream` waits for an event of every session stream that wrote it.
struct UserField {
  const double* ptr = nullptr;
  int64_t ld = 0;
  bool on_device = false;
  hipStream_t stream = nullptr;
  UserField() = default;
  UserField(const double* host) : ptr(host) {}  // a dense host array
  explicit operator bool() const { return ptr != nullptr; }
  int64_t stride(int N) const { return ld ? ld : int64_t(N) + 1; }  // the row stride in elements
};

struct SessionConfig {
  ProblemSpec spec;
  GpuOptions opt;
  Split split = Split::kReference;
  CommKind comm = CommKind::kSelf;
  int world = 1;                 // total ranks (subdomains)
  std::vector<int> ranks;        // ranks owned by this process (default: all for self/local)
  std::vector<int> devices;      // device per owned rank (default: opt.device)
  std::string rccl_uid;          // for kRccl
  std::vector<std::string> ipc_exports;  // for kIpc: every rank's Session::ipc_export(), by rank
  bool rccl_graph = false;       // capture RCCL calls into the hipGraph
  // Build the solvers only; the communicator and driver are created by Session::connect().  A
  // multi-process caller checks that every rank allocated its subdomain before any rank enters
  // the (blocking, collective) RCCL initialisation, so one failing rank cannot hang the others.
  bool defer_connect = false;
  // One host thread (and one driver, graph and stream set) per owned rank: -1 = auto (RCCL with
  // several owned ranks on distinct devices, i.e. `pmx --gpus G`), 1 = always (RCCL only; with a
  // single rank it exercises the threaded path on one GPU), 0 = one host thread drives all ranks.
  int threaded = -1;
  // Subdomains of the whole job that share the busiest device (0 = count this session's own
  // `devices`).  A multi-process job whose ranks share one GPU (bench.py --share-gpu, IPC
  // rehearsals) passes its world size, so every rank sizes the iteration algorithm's fields against
  // the device it shares (choose_algo; the torch path's comm_layout(sharing=...) likewise).
  int sharing = 0;
  // Reaction field c(x, y) >= 0: the session solves (A + (sigma + c) I) u = f.  A global (M+1) x (N+1) fp64
  // array (host or device memory; box-boundary values are ignored and never read), consumed
  // by the constructor.  Runs under the screened problem's rules (apply_sigma_rules) on sessions that own
  // every subdomain; std::invalid_argument, before anything is allocated, otherwise and for a NaN, an
  // infinity or a negative value on an interior node.
  UserField reaction;
  // Diffusion field k(x, y): the session solves (-div(k grad) + sigma + c) u = f.  Nodal values, a global
  // (M+1) x (N+1) fp64 array like `reaction`, but finite and > 0 on EVERY node: the faces next to the box
  // boundary read the boundary values.  Every subdomain keeps the two face-coefficient fields
  // (GpuSubdomainSolver::set_diffusion) and the shift field (filled with sigma when there is no reaction
  // field).  The rules and refusals of `reaction` apply.
  UserField diffusion;
  // Level-set domain: phi(x, y), nodal values like `diffusion`, finite on every node; D = {phi < 0} replaces the
  // ellipse in the face coefficients and in the right-hand-side mask (geometry.hpp: ls_coef_a / ls_coef_b /
  // ls_inside).  The session is a diffusion session -- k = 1 without `diffusion` -- whose face-coefficient
  // fields hold the domain's faces, plus one mask byte per owned node; phi itself is not retained.  The rules and
  // refusals of `diffusion` apply.
  UserField domain;
};

class Session {
 public:
  explicit Session(const SessionConfig& cfg);
  ~Session();
  void connect();  // comm + driver (called by the constructor unless cfg.defer_connect)
  // kIpc (defer_connect): this rank's IPC export; hand every rank's to set_ipc_exports, then connect
  std::string ipc_export();
  void set_ipc_exports(const std::vector<std::string>& e) { cfg_.ipc_exports = e; }
  bool connected() const { return !drivers_.empty(); }

  void init();
  // init from user data: `rhs` replaces the constant F as right-hand side (the solver applies the
  // ellipse mask: B = rhs inside D, 0 elsewhere), `w0` the zero initial iterate (r^0 = B - A w0; its
  // boundary nodes count as 0).  Global (M+1) x (N+1) row-major arrays, either may be null.  Every
  // subdomain gets its block (w0 with its ring, so no exchange of w0 is needed); the data is consumed
  // by this init and not retained: a later init() is the constant-F cold start.  Sessions that own every
  // subdomain (world 1, local communicator) only.
  void init(const double* rhs, const double* w0);
  RunStats solve(const double* rhs, const double* w0, int poll_batches = 1);
  // sqrt(h1 h2 sum (B - A w)^2) over the interior for the w gather_local_w() returns, computed on the
  // device; B from `rhs` ((M+1) x (N+1), null: the constant F) under the ellipse mask.  world == 1.
  double residual_norm(const double* rhs = nullptr);
  // The same three with either field in host or device memory (UserField).  A device field is checked
  // for non-finite values on the device before anything of the session is written
  // (std::invalid_argument, as the bindings raise for a host array), then read in place by the scatter
  // kernel of every subdomain (io_kernels.hip): no staging buffer, nothing retained.  All three have
  // consumed their inputs when they return.  Every subdomain must live on the field's device.
  void init(const UserField& rhs, const UserField& w0);
  RunStats solve(const UserField& rhs, const UserField& w0, int poll_batches = 1);
  double residual_norm(const UserField& rhs);
  // gather_local_w() into device memory: out[gi * ld + gj], (M+1) x (N+1) fp64 with row stride
  // ld >= N + 1, bitwise the host gather -- pending w steps applied, boundary rows and columns zero;
  // elements past column N of a row are not touched.  Stream order as UserField describes for an
  // output on `consumer`; returns without waiting for the kernels.  Sessions that own every subdomain.
  void gather_w_device(double* out, int64_t ld, hipStream_t consumer);
  // The operator on device tensors: out <- alpha L x + beta x + gamma y + c0 on the interior nodes, 0 on the
  // box boundary, L = A + sigma I with the session's sigma -- the plain matrix on the whole box, no ellipse
  // mask.  x, y (may be empty: no y term; may be out's memory) and out are global (M+1) x (N+1) fp64
  // device fields (UserField; out must not overlap x).  Boundary values of x count as 0 and are never
  // loaded.  One k_apply launch per subdomain (apply_kernels.hip), each block reading x across subdomain
  // borders straight from the global array: no exchange.  Evaluated in fp64 whatever the session's storage
  // type.  Stream order as UserField describes: x and y are inputs, out an output on out.stream; returns
  // without waiting.  Touches no field, state or partials of the session; nothing is allocated.
  // std::invalid_argument unless the session owns every subdomain (self / local communicator) on one device.
  void apply_device(const UserField& x, const UserField& out, const UserField& y, double alpha, double beta,
                    double gamma, double c0);
  // Replace the reaction field of a session built with one (SessionConfig::reaction): checked like the
  // constructor's before the session is touched, then every subdomain rewrites its shift field in place
  // (GpuSubdomainSolver::set_reaction) -- same addresses, so the captured graphs stay valid.  The iteration
  // state belongs to the old operator afterwards: step() throws until the next init() / solve().
  void set_reaction(const UserField& c);
  bool has_reaction() const { return bool(cfg_.reaction); }
  // Replace the diffusion field of a session built with one (SessionConfig::diffusion): as set_reaction --
  // checked before the session is touched, the face-coefficient fields rewritten in place, step() throws
  // until the next init() / solve().
  void set_diffusion(const UserField& k);
  bool has_diffusion() const { return bool(cfg_.diffusion); }
  // Replace the domain of a session built with one (SessionConfig::domain), and with it the diffusion field (k
  // empty: k = 1): both checked before the session is touched, the face-coefficient fields and the mask rewritten
  // in place, step() throws until the next init() / solve().  set_diffusion on such a session throws: the
  // geometry is not retained, so the faces cannot be refolded from k alone.
  void set_domain(const UserField& phi, const UserField& k);
  bool has_domain() const { return bool(cfg_.domain); }
  void step(int64_t n);
  void synchronize();
  RunStats solve(int poll_batches = 1);
  // solve with periodic checkpoints to `save_path` (every `every` iterations; none if empty or
  // every == 0), optionally continuing from `resume_path` instead of starting from w = 0
  RunStats solve_checkpointed(const std::string& save_path, int64_t every,
                              const std::string& resume_path, int poll_batches = 1);
  // One file per owned subdomain: `path` when world == 1, else `path.rank<r>`.
  void save_checkpoint(const std::string& path);
  void load_checkpoint(const std::string& path);
  std::string checkpoint_file(const std::string& path, int rank) const;
  // checkpoints do not record ProblemSpec::sigma or a reaction field: std::invalid_argument with either
  void require_no_sigma(const char* what) const;
  RunStats profile(int64_t n);  // threaded: every bucket is the MAX over the owned ranks
  PcgState state(int i = 0);
  bool threaded() const { return threaded_; }  // one host thread per owned rank
  // capture every graph step(n) would replay now, without running (PcgDriver::prepare)
  bool prepare(int64_t n);
  void step_eager(int64_t n);  // n iterations as individual launches (canary)
  PcgDriver::PathStats path_stats() const;
  void reset_path_stats();
  bool split_sweep() const;
  bool direct_rows() const;
  // host-mapped device progress of owned rank i (GpuSubdomainSolver::progress); no HIP call
  void progress(int i, long long out[3]) const;
  // error vs the analytic solution over the owned subdomains (sum of e^2, max |e|, max w)
  ErrorStats error_norms();

  const ProcGrid& grid() const { return pg_; }
  int num_local() const { return int(solvers_.size()); }
  GpuSubdomainSolver& solver(int i) { return *solvers_.at(size_t(i)); }
  const std::string comm_name() const { return comm_ ? comm_->name() : "unconnected"; }
  // the iteration algorithm the solvers run: "ca" (s-step PCG), "pcg1" or "pcg2"
  std::string algo_name() const {
    return solvers_[0]->ca() ? "ca" : solvers_[0]->single_pass() ? "pcg1" : "pcg2";
  }
  bool overlapped() const { return !drivers_.empty() && drivers_[0]->overlapped(); }
  bool poisoned() const { return !drivers_.empty() && drivers_[0]->poisoned(); }
  size_t device_bytes() const;
  // global (M+1) x (N+1) solution filled with the subdomains owned by this process
  std::vector<double> gather_local_w();
  // local interior (nx x ny, row-major) of owned subdomain i
  std::vector<double> local_w(int i = 0);
  // the per-tile partial sums (5 per tile slot) the last sweep wrote (tests of the reduction hand-off)
  std::vector<double> partials(int i = 0);
  hipStream_t stream_of(int i) const;  // the compute stream of owned rank i

 private:
  void require_connected() const {
    PMX_CHECK(!drivers_.empty(), "session not connected (Session::connect)");
  }
  // f(driver index, driver) for every driver: inline, or one host thread per driver (each bound
  // to its rank's device) in threaded mode; the first exception is rethrown after all joined
  void for_drivers(const std::function<void(size_t, PcgDriver&)>& f);
  RunStats solve_impl(int poll_batches, bool do_init, int64_t every, const std::string& save_path);
  // GpuSubdomainSolver::set_init_data / set_init_data_device on every solver
  void stage_init_data(const UserField& rhs, const UserField& w0);
  void require_owns_all(const char* what) const;  // self / local communicator
  int require_one_device() const;        // the device every solver lives on (device fields need one)
  void wait_for(hipStream_t producer);   // every session stream waits for `producer`'s work so far
  void hand_over(hipStream_t consumer);  // `consumer` waits for every session stream's work so far
  // One field under its value rule (pmx/operator.hpp); name: what the refusal calls it
  struct FieldCheck {
    const UserField* f;
    FieldRule rule;
    const char* name;
  };
  // throws std::invalid_argument ("<name>" + field_rule_text) for the first field of the list that breaks its
  // rule.  Host fields: field_values_ok.  Device fields (memory of `device`): one flag each in one allocation,
  // one launch_value_check each on s, one copy back and one synchronise.  Empty fields are skipped.
  void check_values(std::initializer_list<FieldCheck> fields, int device, hipStream_t s) const;
  // the device fields among rhs and w0, on stream_of(0)
  void check_finite(const UserField& rhs, const UserField& w0);
  // a reaction, diffusion or level-set field of the constructor or a set_*: its row stride, then its values
  // under `rule` -- a device field on its producer's stream, and only with every subdomain on its device
  void check_coefficient(const UserField& f, FieldRule rule, const std::string& name) const;
  // set_reaction / set_diffusion: the field checked, the session idle, the upload, the iteration state stale
  void set_coefficient(const UserField& f, bool diffusion);
  void upload_reaction(const UserField& c);
  // a host field goes up whole to a temporary device copy per subdomain, so that one kernel forms the face
  // fields from either source (the same bits)
  void upload_diffusion(const UserField& k);
  // the same for a level-set domain: phi, and k where there is one (empty: k = 1)
  void upload_domain(const UserField& phi, const UserField& k);
  // what the refusals call the session's coefficient field; nullptr without one
  const char* field_noun() const {
    return has_domain()      ? "a level-set domain"
           : has_diffusion() ? "a diffusion field"
           : has_reaction()  ? "a reaction field"
                             : nullptr;
  }
  bool stale_ = false;  // set_reaction since the last init: the iteration state is the old operator's

  SessionConfig cfg_;
  ProcGrid pg_;
  std::vector<std::unique_ptr<GpuSubdomainSolver>> solvers_;
  std::unique_ptr<Comm> comm_;
  std::vector<std::unique_ptr<Comm>> views_;            // threaded: per-rank communicators
  std::vector<std::unique_ptr<PcgDriver>> drivers_;     // one (all ranks) or one per rank
  bool threaded_ = false;
};

// Largest square grid whose fields fit into `bytes_per_gpu` on `gpus` devices (SURVEY §5.7:
// subgrids sized against 288 GB HBM per MI355X): the default single pass keeps 5 fields, 8 B/pt
// each in fp64 and 4 B/pt in fp32.
// Every rank's communication calls for `iters` iterations of its own driver on a RecordingComm (all
// ranks on the current device of opt.device, nothing exchanged): the test that every rank issues the
// same sequence of collectives and matching send/recv groups per captured batch.
std::vector<std::vector<CommEvent>> record_comm_sequence(const ProblemSpec& spec, int world, Split split,
                                                         const GpuOptions& opt, int64_t iters);

int64_t max_square_grid(double bytes_per_gpu, int gpus, DType dtype, double reserve_fraction = 0.1, int algo = -1);

}  // namespace pmx
