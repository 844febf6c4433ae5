// Session: decomposition + solvers + comm + driver.  See pmx/session.hpp.
#include "pmx/session.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <exception>
#include <fstream>
#include <mutex>
#include <set>
#include <stdexcept>
#include <thread>

#include "pmx/common.hpp"

namespace pmx {

Session::Session(const SessionConfig& cfg) : cfg_(cfg) {
  cfg_.spec.validate();
  PMX_CHECK(cfg_.world >= 1, "world size must be >= 1");
  pg_ = make_process_grid(cfg_.world, cfg_.spec.M, cfg_.spec.N, cfg_.split);
  if (cfg_.ranks.empty()) {
    if (cfg_.comm == CommKind::kRccl) {
      PMX_CHECK(false, "RCCL sessions must list the ranks they own");
    }
    for (int r = 0; r < cfg_.world; ++r) cfg_.ranks.push_back(r);
  }
  if (cfg_.devices.empty()) cfg_.devices.assign(cfg_.ranks.size(), cfg_.opt.device);
  PMX_CHECK(cfg_.devices.size() == cfg_.ranks.size(), "one device per owned rank");
  if (cfg_.comm == CommKind::kSelf)
    PMX_CHECK(cfg_.world == 1, "self comm needs world == 1 (use local or rccl)");
  if (cfg_.comm == CommKind::kLocal)
    PMX_CHECK(int(cfg_.ranks.size()) == cfg_.world, "local comm owns every rank");
  if (cfg_.comm == CommKind::kIpc)
    PMX_CHECK(cfg_.ranks.size() == 1, "the IPC transport runs one rank per process");
  if (cfg_.comm == CommKind::kLoopback)
    PMX_CHECK(cfg_.ranks.size() == 1, "loopback runs exactly one rank of the decomposition");

  // one iteration algorithm for every subdomain (and every process: the choice only depends on
  // global data, see choose_algo)
  GpuOptions pre = cfg_.opt;
  // a multi-process RCCL run tracks device progress for its hang watchdog (GpuOptions::progress)
  if ((cfg_.comm == CommKind::kRccl || cfg_.comm == CommKind::kIpc) && cfg_.world > 1) pre.progress = 1;
  const UserField &react = cfg_.reaction, &dif = cfg_.diffusion, &dom = cfg_.domain;
  if (react || dif || dom) {
    if (cfg_.comm != CommKind::kSelf && cfg_.comm != CommKind::kLocal)
      throw std::invalid_argument(std::string(react ? "a reaction field" : dif ? "a diffusion field"
                                                                               : "a level-set domain") +
                                  " needs a session that owns every subdomain (world 1 or the local communicator); "
                                  "multi-process transports are not supported");
    pre.shift_field = 1;  // T(sigma + c), c = 0 without a reaction field
    pre.diffusion = dif || dom ? 1 : 0;  // a domain session is a diffusion session, k = 1 without a field
    pre.domain = dom ? 1 : 0;
  }
  GpuOptions base = resolve_options(pre);
  // sigma != 0 or a reaction field: pcg1 on the row march, or std::invalid_argument
  apply_sigma_rules(cfg_.spec, pg_, base);
  if (react) check_coefficient(react, FieldRule::kNonNegInterior, "reaction");  // before anything is allocated
  if (dif) check_coefficient(dif, FieldRule::kPositive, "diffusion");
  if (dom) check_coefficient(dom, FieldRule::kFinite, "domain");
  if (base.algo == -1) {
    HIP_CHECK(hipSetDevice(cfg_.devices[0]));
    size_t free_b = 0, total_b = 0;
    HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    int per_device = 0;  // subdomains sharing the busiest device
    for (int d : cfg_.devices) per_device = std::max<int>(per_device, int(std::count(cfg_.devices.begin(), cfg_.devices.end(), d)));
    per_device = std::max(per_device, cfg_.sharing);
    // every transport of a Session moves ghost rows straight between the fields (direct rows)
    base.algo = choose_algo(cfg_.spec, pg_, base, double(total_b), per_device, true);
  }
  for (size_t i = 0; i < cfg_.ranks.size(); ++i) {
    GpuOptions o = base;
    o.device = cfg_.devices[i];
    if (cfg_.comm == CommKind::kLoopback) o.ca_dirichlet = 1;  // see GpuOptions::ca_dirichlet
    const Subdomain sd = decompose_2d(cfg_.spec.M, cfg_.spec.N, pg_, cfg_.ranks[i]);
    solvers_.push_back(std::make_unique<GpuSubdomainSolver>(cfg_.spec, sd, o));
  }
  if (react) upload_reaction(react);
  if (dif || dom) {
    if (!react) {  // the shift field of a diffusion session without a reaction field: T(sigma)
      const std::vector<double> zero(size_t(cfg_.spec.M + 1) * size_t(cfg_.spec.N + 1), 0.0);
      upload_reaction(UserField(zero.data()));
    }
    if (dom) upload_domain(dom, dif);
    else upload_diffusion(dif);
  }
  if (!cfg_.defer_connect) connect();
}

std::string Session::ipc_export() {
  PMX_CHECK(cfg_.comm == CommKind::kIpc, "ipc_export needs an IPC session");
  if (!comm_) comm_ = make_ipc_comm(solvers_[0].get(), cfg_.world);
  return pmx::ipc_export(comm_.get());
}

void Session::connect() {
  PMX_CHECK(drivers_.empty(), "session already connected");
  std::vector<GpuSubdomainSolver*> raw;
  for (auto& s : solvers_) raw.push_back(s.get());
  switch (cfg_.comm) {
    case CommKind::kIpc:
      if (!comm_) comm_ = make_ipc_comm(raw[0], cfg_.world);
      if (cfg_.world == 1 && cfg_.ipc_exports.empty()) cfg_.ipc_exports.push_back(pmx::ipc_export(comm_.get()));
      ipc_attach(comm_.get(), cfg_.ipc_exports);
      break;
    case CommKind::kSelf: comm_ = make_self_comm(); break;
    case CommKind::kLoopback: comm_ = make_loopback_comm(); break;
    case CommKind::kLocal: comm_ = make_local_comm(raw); break;
    case CommKind::kRccl:
      // overlap off = the serialized schedule: one communicator, every call on the compute stream
      comm_ = make_rccl_comm(cfg_.rccl_uid, cfg_.world, cfg_.ranks, cfg_.devices, cfg_.rccl_graph, cfg_.opt.overlap);
      break;
  }
  // one host thread per GPU.  Several owned ranks on distinct devices (pmx --gpus G)
  // get a driver each -- own streams, own graph captured by its own thread -- so no device's
  // launches queue behind another's on one host thread.
  const std::set<int> devs(cfg_.devices.begin(), cfg_.devices.end());
  const bool auto_threads = cfg_.comm == CommKind::kRccl && raw.size() > 1 && devs.size() == raw.size();
  threaded_ = cfg_.threaded == 1 || (cfg_.threaded == -1 && auto_threads);
  PMX_CHECK(!threaded_ || cfg_.comm == CommKind::kRccl, "threaded drivers need the RCCL communicator");
  if (!threaded_) {
    drivers_.push_back(std::make_unique<PcgDriver>(raw, comm_.get(), cfg_.opt.graph_batch));
    return;
  }
  for (size_t i = 0; i < raw.size(); ++i) {
    views_.push_back(comm_->rank_view(int(i)));
    HIP_CHECK(hipSetDevice(raw[i]->device()));
    drivers_.push_back(std::make_unique<PcgDriver>(std::vector<GpuSubdomainSolver*>{raw[i]}, views_.back().get(),
                                                   cfg_.opt.graph_batch));
  }
}

Session::~Session() {
  drivers_.clear();
  views_.clear();
  comm_.reset();
  solvers_.clear();
}

void Session::for_drivers(const std::function<void(size_t, PcgDriver&)>& f) {
  require_connected();
  if (!threaded_) {
    f(0, *drivers_[0]);
    return;
  }
  std::exception_ptr err;
  std::mutex mu;
  std::vector<std::thread> th;
  th.reserve(drivers_.size());
  for (size_t i = 0; i < drivers_.size(); ++i)
    th.emplace_back([&, i] {
      try {
        HIP_CHECK(hipSetDevice(solvers_[i]->device()));
        f(i, *drivers_[i]);
      } catch (...) {
        bool first = false;
        {
          std::lock_guard<std::mutex> lk(mu);
          if (!err) {
            err = std::current_exception();
            first = true;
          }
        }
        // The other threads may be blocked on collectives this rank will never post: abort the
        // communicator so they return with an error and the join below cannot hang.
        if (first && comm_) comm_->abort();
      }
    });
  for (auto& t : th) t.join();
  if (err) std::rethrow_exception(err);
}

hipStream_t Session::stream_of(int i) const {
  require_connected();
  return threaded_ ? drivers_.at(size_t(i))->streams()[0] : drivers_[0]->streams().at(size_t(i));
}

bool Session::prepare(int64_t n) {
  std::vector<char> ok(drivers_.size(), 0);
  for_drivers([&](size_t i, PcgDriver& d) { ok[i] = d.prepare(n) ? 1 : 0; });
  bool all = true;
  for (char c : ok) all &= c != 0;
  return all;
}

void Session::step_eager(int64_t n) {
  for_drivers([n](size_t, PcgDriver& d) { d.enqueue_eager(n); });
}

PcgDriver::PathStats Session::path_stats() const {
  require_connected();
  PcgDriver::PathStats p = drivers_[0]->path_stats();
  for (auto& d : drivers_)
    PMX_CHECK(d->path_stats().graph_iters == p.graph_iters && d->path_stats().eager_iters == p.eager_iters,
              "drivers disagree on the launch path");
  return p;
}

void Session::reset_path_stats() {
  for (auto& d : drivers_) d->reset_path_stats();
}

bool Session::split_sweep() const {
  require_connected();
  return drivers_[0]->split_sweep();
}

bool Session::direct_rows() const {
  require_connected();
  return drivers_[0]->direct_rows();
}

void Session::progress(int i, long long out[3]) const { solvers_.at(size_t(i))->progress(out); }

void Session::check_values(std::initializer_list<FieldCheck> fields, int device, hipStream_t s) const {
  const int M = cfg_.spec.M, N = cfg_.spec.N;
  std::vector<int> h(fields.size(), 0);  // device fields: the flag of each
  auto on_device = [](const FieldCheck& c) { return *c.f && c.f->on_device; };
  if (std::any_of(fields.begin(), fields.end(), on_device)) {
    HIP_CHECK(hipSetDevice(device));
    int* raw = nullptr;  // for the call only
    HIP_CHECK(hipMalloc(&raw, h.size() * sizeof(int)));
    const DevPtr<int> flag(raw);
    HIP_CHECK(hipMemsetAsync(flag.get(), 0, h.size() * sizeof(int), s));
    size_t q = 0;
    for (const FieldCheck& c : fields) {
      if (on_device(c)) launch_value_check(c.rule, c.f->ptr, c.f->stride(N), M, N, flag.get() + q, s);
      ++q;
    }
    HIP_CHECK(hipMemcpyAsync(h.data(), flag.get(), h.size() * sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
  }
  size_t q = 0;
  for (const FieldCheck& c : fields) {
    const bool ok = !*c.f || (c.f->on_device ? h[q] == 0 : field_values_ok(c.f->ptr, c.f->stride(N), M, N, c.rule));
    if (!ok) throw std::invalid_argument(std::string(c.name) + field_rule_text(c.rule));
    ++q;
  }
}

void Session::check_coefficient(const UserField& f, FieldRule rule, const std::string& name) const {
  if (f.stride(cfg_.spec.N) < cfg_.spec.N + 1) throw std::invalid_argument(name + ": row stride below N + 1");
  if (f.on_device)
    for (int d : cfg_.devices)
      if (d != cfg_.devices[0])
        throw std::invalid_argument("a device " + name + " field needs every subdomain of the session on its device");
  check_values({{&f, rule, name.c_str()}}, cfg_.devices[0], f.stream);
}

void Session::upload_reaction(const UserField& c) {
  // a device field on its producer's stream (ordered after its producer, no event needed); every solver
  // returns once that stream has consumed the field
  for (auto& sp : solvers_)
    sp->set_reaction(c.ptr, c.stride(cfg_.spec.N), c.on_device, c.on_device ? c.stream : nullptr);
}

void Session::upload_diffusion(const UserField& k) {
  const int M = cfg_.spec.M, N = cfg_.spec.N;
  for (auto& sp : solvers_) {
    if (k.on_device) {  // on its producer's stream; the solver returns once that stream has consumed the field
      sp->set_diffusion(k.ptr, k.stride(N), k.stream);
      continue;
    }
    HIP_CHECK(hipSetDevice(sp->device()));
    double* raw = nullptr;  // for this subdomain's kernel only
    HIP_CHECK(hipMalloc(&raw, size_t(M + 1) * size_t(N + 1) * sizeof(double)));
    const DevPtr<double> tmp(raw);
    HIP_CHECK(hipMemcpy2D(tmp.get(), size_t(N + 1) * sizeof(double), k.ptr, size_t(k.stride(N)) * sizeof(double),
                          size_t(N + 1) * sizeof(double), size_t(M + 1), hipMemcpyHostToDevice));
    sp->set_diffusion(tmp.get(), N + 1, nullptr);
  }
}

namespace {

// A global field for a setup kernel of device `device`: a device field as it is, a host field as a dense
// temporary device copy that lives as long as the object.
struct OnDevice {
  DevPtr<double> tmp;
  const double* ptr = nullptr;
  int64_t ld = 0;
  OnDevice(const UserField& f, int M, int N, int device) {
    if (!f) return;
    ld = f.stride(N);
    ptr = f.ptr;
    if (f.on_device) return;
    HIP_CHECK(hipSetDevice(device));
    double* raw = nullptr;
    HIP_CHECK(hipMalloc(&raw, size_t(M + 1) * size_t(N + 1) * sizeof(double)));
    tmp.reset(raw);
    HIP_CHECK(hipMemcpy2D(raw, size_t(N + 1) * sizeof(double), f.ptr, size_t(ld) * sizeof(double),
                          size_t(N + 1) * sizeof(double), size_t(M + 1), hipMemcpyHostToDevice));
    ptr = raw;
    ld = N + 1;
  }
};

}  // namespace

void Session::upload_domain(const UserField& phi, const UserField& k) {
  const int M = cfg_.spec.M, N = cfg_.spec.N;
  // the kernel runs on phi's stream (a host phi: the null stream, after the blocking copies); a device k of
  // another stream has been consumed up to here by its value check, which waits for that stream
  if (k && k.on_device && !(phi.on_device && phi.stream == k.stream)) HIP_CHECK(hipStreamSynchronize(k.stream));
  for (auto& sp : solvers_) {
    const OnDevice p(phi, M, N, sp->device()), q(k, M, N, sp->device());
    sp->set_domain(p.ptr, p.ld, q.ptr, q.ld, phi.on_device ? phi.stream : nullptr);
  }
}

void Session::set_domain(const UserField& phi, const UserField& k) {
  if (!has_domain())
    throw std::invalid_argument("set_domain needs a session built with a level-set domain (make_session(p, "
                                "domain=phi)): sessions without one hold no right-hand-side mask");
  if (!phi) throw std::invalid_argument("set_domain: no field given");
  check_coefficient(phi, FieldRule::kFinite, "domain");
  if (k) check_coefficient(k, FieldRule::kPositive, "diffusion");
  if (!drivers_.empty()) synchronize();  // no sweep in flight reads the fields
  upload_domain(phi, k);
  cfg_.domain = phi;  // (kept as flags: has_domain / has_diffusion; the memory is the caller's)
  cfg_.diffusion = k;
  stale_ = true;
}

void Session::set_coefficient(const UserField& f, bool diffusion) {
  const std::string name = diffusion ? "diffusion" : "reaction";
  if (diffusion && has_domain())
    throw std::invalid_argument("set_diffusion: the session was built with a level-set domain, whose geometry is not "
                                "retained, so the faces cannot be refolded from k alone; call set_domain(phi, "
                                "diffusion=k)");
  if (!(diffusion ? has_diffusion() : has_reaction()))
    throw std::invalid_argument("set_" + name + " needs a session built with a " + name + " field (make_session(p, " +
                                name + (diffusion ? "=k" : "=c") + ")): sessions without one hold no " +
                                (diffusion ? "face-coefficient fields" : "shift field"));
  if (!f) throw std::invalid_argument("set_" + name + ": no field given");
  check_coefficient(f, diffusion ? FieldRule::kPositive : FieldRule::kNonNegInterior, name);
  if (!drivers_.empty()) synchronize();  // no sweep in flight reads the fields
  if (diffusion) upload_diffusion(f);
  else upload_reaction(f);
  stale_ = true;
}

void Session::set_reaction(const UserField& c) { set_coefficient(c, false); }
void Session::set_diffusion(const UserField& k) { set_coefficient(k, true); }

ErrorStats Session::error_norms() {
  if (const char* noun = field_noun())
    throw std::invalid_argument(std::string("error_norms: the closed-form solution does not solve a problem with ") +
                                noun + "; compare the solution with your own (PoissonEllipse.error_norms(w, exact=u))");
  if (cfg_.spec.sigma != 0.0)
    throw std::invalid_argument("error_norms: the closed-form solution holds for sigma = 0 only; compare the "
                                "solution with your own (PoissonEllipse.error_norms(w, exact=u))");
  synchronize();
  ErrorStats t;
  t.max_w = -HUGE_VAL;
  for (size_t i = 0; i < solvers_.size(); ++i) {
    const ErrorStats e = solvers_[i]->error_norms(stream_of(int(i)));
    t.sum_e2 += e.sum_e2;
    t.max_e = std::max(t.max_e, e.max_e);
    t.max_w = std::max(t.max_w, e.max_w);
  }
  return t;
}

void Session::init() {
  stale_ = false;
  for_drivers([](size_t, PcgDriver& d) { d.init(); });
}

void Session::require_owns_all(const char* what) const {
  PMX_CHECK(cfg_.comm == CommKind::kSelf || cfg_.comm == CommKind::kLocal,
            what << " needs a session that owns every subdomain (world 1 or the "
            "local communicator); multi-process sessions are not supported");
}

int Session::require_one_device() const {
  const int dev = solvers_[0]->device();
  for (auto& sp : solvers_)
    PMX_CHECK(sp->device() == dev, "device fields need every subdomain of the session on one device");
  return dev;
}

void Session::wait_for(hipStream_t producer) {
  HIP_CHECK(hipSetDevice(require_one_device()));
  hipEvent_t e = nullptr;
  HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  hipError_t err = hipEventRecord(e, producer);
  for (size_t i = 0; i < solvers_.size() && err == hipSuccess; ++i) err = hipStreamWaitEvent(stream_of(int(i)), e, 0);
  (void)hipEventDestroy(e);  // released once the waits enqueued above have passed it
  HIP_CHECK(err);
}

void Session::check_finite(const UserField& rhs, const UserField& w0) {
  const UserField none, &f = rhs.on_device ? rhs : none, &w = w0.on_device ? w0 : none;  // host fields: the caller's
  if (!f && !w) return;
  check_values({{&f, FieldRule::kFinite, "rhs"}, {&w, FieldRule::kFinite, "w0"}}, require_one_device(), stream_of(0));
}

void Session::stage_init_data(const UserField& rhs, const UserField& w0) {
  if (!rhs && !w0) return;
  require_owns_all("a right-hand side / initial guess");
  // device fields: ordered after their producers' work, and checked before the session is touched
  for (const UserField* f : {&rhs, &w0}) {
    if (!*f || !f->on_device) continue;
    PMX_CHECK(f->ld == 0 || f->ld >= cfg_.spec.N + 1, "row stride of a device field below N + 1");
    if (f == &w0 && rhs && rhs.on_device && rhs.stream == w0.stream) continue;  // one wait serves both
    wait_for(f->stream);
  }
  check_finite(rhs, w0);
  // every subdomain reads its block straight out of the global arrays (row stride N + 1 unless the
  // field says otherwise): f from its first owned node, w0 one node earlier in both directions, i.e.
  // with its ring -- the neighbours' values, so nothing is exchanged for w0
  const int64_t ldf = rhs.stride(cfg_.spec.N), ldw = w0.stride(cfg_.spec.N);
  for (auto& sp : solvers_) {
    const Subdomain& sd = sp->sd();
    // local (0, 0) of w0, the first owned node of rhs
    const double* f = rhs ? rhs.ptr + (int64_t(sd.gi0()) + 1) * ldf + sd.gj0() + 1 : nullptr;
    const double* w = w0 ? w0.ptr + int64_t(sd.gi0()) * ldw + sd.gj0() : nullptr;
    sp->set_init_data(rhs.on_device ? nullptr : f, w0.on_device ? nullptr : w, ldf, ldw);
    sp->set_init_data_device(rhs.on_device ? f : nullptr, w0.on_device ? w : nullptr, ldf, ldw);
  }
}

void Session::init(const UserField& rhs, const UserField& w0) {
  require_connected();
  stage_init_data(rhs, w0);
  init();
}

RunStats Session::solve(const UserField& rhs, const UserField& w0, int poll_batches) {
  require_connected();
  stage_init_data(rhs, w0);
  return solve(poll_batches);
}

void Session::init(const double* rhs, const double* w0) { init(UserField(rhs), UserField(w0)); }

RunStats Session::solve(const double* rhs, const double* w0, int poll_batches) {
  return solve(UserField(rhs), UserField(w0), poll_batches);
}

double Session::residual_norm(const UserField& rhs) {
  PMX_CHECK(cfg_.world == 1, "residual_norm runs undecomposed sessions (world == 1): w has no ghost exchange");
  synchronize();
  if (rhs && rhs.on_device) {
    PMX_CHECK(rhs.ld == 0 || rhs.ld >= cfg_.spec.N + 1, "row stride of a device field below N + 1");
    wait_for(rhs.stream);
    check_finite(rhs, UserField());
  }
  GpuSubdomainSolver& g = *solvers_[0];
  const int64_t ld = rhs.stride(cfg_.spec.N);  // the owned nodes start at global (1, 1)
  const GridInfo gi(cfg_.spec);
  return std::sqrt(gi.h1h2 * g.residual_sumsq(rhs ? rhs.ptr + ld + 1 : nullptr, stream_of(0), ld, rhs.on_device));
}

double Session::residual_norm(const double* rhs) { return residual_norm(UserField(rhs)); }

void Session::gather_w_device(double* out, int64_t ld, hipStream_t consumer) {
  require_connected();
  require_owns_all("a device solution");
  PMX_CHECK(out && ld >= cfg_.spec.N + 1, "gather_w_device needs an (M+1) x (N+1) array with row stride >= N+1");
  synchronize();
  wait_for(consumer);  // earlier work on the consumer's stream may still use `out`
  for (size_t i = 0; i < solvers_.size(); ++i) solvers_[i]->gather_w_device(out, ld, stream_of(int(i)));
  hand_over(consumer);
}

void Session::hand_over(hipStream_t consumer) {
  hipEvent_t e = nullptr;
  HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  hipError_t err = hipSuccess;
  for (size_t i = 0; i < solvers_.size() && err == hipSuccess; ++i) {
    err = hipEventRecord(e, stream_of(int(i)));
    if (err == hipSuccess) err = hipStreamWaitEvent(consumer, e, 0);
  }
  (void)hipEventDestroy(e);
  HIP_CHECK(err);
}

void Session::apply_device(const UserField& x, const UserField& out, const UserField& y, double alpha, double beta,
                           double gamma, double c0) {
  require_connected();
  const int M = cfg_.spec.M, N = cfg_.spec.N;
  if (cfg_.comm != CommKind::kSelf && cfg_.comm != CommKind::kLocal)
    throw std::invalid_argument("apply needs a session that owns every subdomain (world 1 or the local "
                                "communicator); multi-process sessions are not supported");
  for (auto& sp : solvers_)
    if (sp->device() != solvers_[0]->device())
      throw std::invalid_argument("apply needs every subdomain of the session on the tensors' device");
  for (const UserField* f : {&x, &out, &y}) {
    if (f == &y && !y) continue;
    if (!*f || !f->on_device) throw std::invalid_argument("apply: x, out and y are device fields");
    if (f->ld != 0 && f->ld < N + 1) throw std::invalid_argument("apply: row stride of a device field below N + 1");
  }
  if (!(std::isfinite(alpha) && std::isfinite(beta) && std::isfinite(gamma) && std::isfinite(c0)))
    throw std::invalid_argument("apply: alpha, beta, gamma and const must be finite");
  auto ld = [&](const UserField& f) { return f.stride(N); };
  auto span = [&](const UserField& f) { return (int64_t(M) * ld(f) + N + 1) * int64_t(sizeof(double)); };
  const char *xb = reinterpret_cast<const char*>(x.ptr), *ob = reinterpret_cast<const char*>(out.ptr);
  if (xb < ob + span(out) && ob < xb + span(x)) throw std::invalid_argument("apply: out overlaps x");
  if (y && !(y.ptr == out.ptr && ld(y) == ld(out))) {  // out may BE y: every lane reads its element before writing it
    const char* yb = reinterpret_cast<const char*>(y.ptr);
    if (yb < ob + span(out) && ob < yb + span(y)) throw std::invalid_argument("apply: out overlaps y without being y");
  }

  // inputs after their producers' work, and after whatever the consumer's stream still does with out
  wait_for(x.stream);
  if (y && y.stream != x.stream) wait_for(y.stream);
  if (out.stream != x.stream && !(y && out.stream == y.stream)) wait_for(out.stream);
  ApplyCoef K;
  K.alpha = alpha; K.beta = beta; K.gamma = y ? gamma : 0.0; K.c0 = c0;
  K.plain = alpha == 1.0 && beta == 0.0 && !y && c0 == 0.0;
  for (size_t i = 0; i < solvers_.size(); ++i) {
    // sigma, or the owning subdomain's shift field in its place and its face-coefficient fields in the tables'
    set_operator(K, solvers_[i]->op<void>());
    if (K.shift) {
      K.spitch = solvers_[i]->pitch();
      K.sgi0 = solvers_[i]->sd().gi0();
      K.sgj0 = solvers_[i]->sd().gj0();
      K.selem = int(solvers_[i]->elem_bytes());
    }
    // the owned nodes, widened by the global boundary row / column where the block touches it (as k_gather)
    const Subdomain& sd = solvers_[i]->sd();
    const int i0 = sd.gi0() == 0 ? 0 : sd.gi0() + 1, i1 = sd.gi0() + sd.nx + 1 == M ? M : sd.gi0() + sd.nx;
    const int j0 = sd.gj0() == 0 ? 0 : sd.gj0() + 1, j1 = sd.gj0() + sd.ny + 1 == N ? N : sd.gj0() + sd.ny;
    launch_apply(solvers_[i]->geom(), solvers_[i]->tables(), x.ptr, ld(x), y.ptr, y ? ld(y) : 0,
                 const_cast<double*>(out.ptr), ld(out), i0, j0, i1 - i0 + 1, j1 - j0 + 1, K, stream_of(int(i)));
  }
  hand_over(out.stream);
}

void Session::step(int64_t n) {
  PMX_CHECK(!stale_, "step: the reaction or diffusion field or the domain changed (set_reaction / set_diffusion / "
                     "set_domain) since the last init; call init() or solve()");
  for_drivers([n](size_t, PcgDriver& d) { d.enqueue_iterations(n); });
}

void Session::synchronize() {
  for_drivers([](size_t, PcgDriver& d) { d.synchronize(); });
}

PcgState Session::state(int i) {
  require_connected();
  return threaded_ ? drivers_.at(size_t(i))->state(0) : drivers_[0]->state(i);
}

RunStats Session::solve_impl(int poll_batches, bool do_init, int64_t every, const std::string& save_path) {
  // every rank's driver iterates to the same device stop decision (the all-reduced scalars are
  // identical everywhere); rank 0's statistics are returned
  std::vector<RunStats> st(drivers_.size());
  if (do_init) stale_ = false;
  PMX_CHECK(!stale_, "the reaction or diffusion field or the domain changed (set_reaction / set_diffusion / "
                     "set_domain) since the last init; call init() or solve()");
  for_drivers([&](size_t i, PcgDriver& d) {
    std::function<void(const PcgState&)> cb;
    if (every > 0 && !save_path.empty()) {
      cb = [&, i](const PcgState&) {
        if (!threaded_) {
          save_checkpoint(save_path);
          return;
        }
        const std::string f = checkpoint_file(save_path, solvers_[i]->sd().rank), tmp = f + ".tmp";
        {
          std::ofstream os(tmp, std::ios::binary | std::ios::trunc);
          PMX_CHECK(os.good(), "cannot open checkpoint file " << tmp);
          solvers_[i]->save_checkpoint(os, d.streams()[0]);
        }
        PMX_CHECK(std::rename(tmp.c_str(), f.c_str()) == 0, "cannot rename " << tmp << " -> " << f);
      };
    }
    st[i] = d.solve(poll_batches, do_init, every, cb);
  });
  for (const RunStats& r : st)
    PMX_CHECK(r.iters == st[0].iters && r.status == st[0].status,
              "ranks disagree on the stop decision (" << r.iters << " vs " << st[0].iters << " iterations)");
  return st[0];
}

RunStats Session::solve(int poll_batches) { return solve_impl(poll_batches, true, 0, ""); }

RunStats Session::profile(int64_t n) {
  std::vector<RunStats> st(drivers_.size());
  for_drivers([&](size_t i, PcgDriver& d) { st[i] = d.profile_phases(n); });
  RunStats m = st[0];
  for (const RunStats& r : st) {  // MAX over ranks, as the reference reports its buckets
    m.t_kernel_a = std::max(m.t_kernel_a, r.t_kernel_a);
    m.t_kernel_b = std::max(m.t_kernel_b, r.t_kernel_b);
    m.t_reduce = std::max(m.t_reduce, r.t_reduce);
    m.t_allreduce = std::max(m.t_allreduce, r.t_allreduce);
    m.t_halo = std::max(m.t_halo, r.t_halo);
    m.t_comm = std::max(m.t_comm, r.t_comm);
  }
  return m;
}

size_t Session::device_bytes() const {
  size_t b = 0;
  for (auto& s : solvers_) b += s->device_bytes();
  return b;
}

std::vector<double> Session::local_w(int i) {
  synchronize();
  return solvers_.at(size_t(i))->download_w(stream_of(i));
}

std::vector<double> Session::partials(int i) {
  synchronize();
  return solvers_.at(size_t(i))->read_partials(stream_of(i));
}

std::vector<double> Session::gather_local_w() {
  const int M = cfg_.spec.M, N = cfg_.spec.N;
  std::vector<double> g(size_t(M + 1) * (N + 1), 0.0);
  for (size_t i = 0; i < solvers_.size(); ++i) {
    auto& s = *solvers_[i];
    const Subdomain& sd = s.sd();
    const std::vector<double> w = s.download_w(stream_of(int(i)));
    for (int li = 1; li <= sd.nx; ++li)
      for (int lj = 1; lj <= sd.ny; ++lj)
        g[size_t(sd.gi0() + li) * (N + 1) + sd.gj0() + lj] = w[size_t(li - 1) * sd.ny + lj - 1];
  }
  return g;
}

void Session::require_no_sigma(const char* what) const {
  if (const char* noun = field_noun())
    throw std::invalid_argument(std::string(what) + ": checkpoint files do not record " + noun +
                                " (format v7); sessions with one cannot be checkpointed");
  if (cfg_.spec.sigma != 0.0)
    throw std::invalid_argument(std::string(what) + ": checkpoint files do not record sigma (format v7); "
                                "sessions with sigma != 0 cannot be checkpointed");
}

std::string Session::checkpoint_file(const std::string& path, int rank) const {
  return cfg_.world == 1 ? path : path + ".rank" + std::to_string(rank);
}

void Session::save_checkpoint(const std::string& path) {
  require_no_sigma("save_checkpoint");
  synchronize();
  for (size_t i = 0; i < solvers_.size(); ++i) {
    const std::string f = checkpoint_file(path, solvers_[i]->sd().rank);
    const std::string tmp = f + ".tmp";
    {
      std::ofstream os(tmp, std::ios::binary | std::ios::trunc);
      PMX_CHECK(os.good(), "cannot open checkpoint file " << tmp);
      solvers_[i]->save_checkpoint(os, stream_of(int(i)));
    }
    PMX_CHECK(std::rename(tmp.c_str(), f.c_str()) == 0, "cannot rename " << tmp << " -> " << f);
  }
}

void Session::load_checkpoint(const std::string& path) {
  require_no_sigma("load_checkpoint");
  synchronize();
  for (size_t i = 0; i < solvers_.size(); ++i) {
    const std::string f = checkpoint_file(path, solvers_[i]->sd().rank);
    std::ifstream is(f, std::ios::binary);
    PMX_CHECK(is.good(), "cannot open checkpoint file " << f);
    solvers_[i]->load_checkpoint(is, stream_of(int(i)));
  }
}

RunStats Session::solve_checkpointed(const std::string& save_path, int64_t every,
                                     const std::string& resume_path, int poll_batches) {
  require_no_sigma("solve_checkpointed");
  const bool resume = !resume_path.empty();
  if (resume) load_checkpoint(resume_path);
  return solve_impl(poll_batches, !resume, every, save_path);
}

std::vector<std::vector<CommEvent>> record_comm_sequence(const ProblemSpec& spec, int world, Split split,
                                                         const GpuOptions& opt, int64_t iters) {
  const ProcGrid pg = make_process_grid(world, spec.M, spec.N, split);
  GpuOptions o = resolve_options(opt);
  apply_sigma_rules(spec, pg, o);
  if (o.algo == -1) o.algo = choose_algo(spec, pg, o, 0.0, world, true);
  std::vector<std::unique_ptr<GpuSubdomainSolver>> solvers;
  std::vector<std::vector<CommEvent>> logs(static_cast<size_t>(world));
  std::vector<std::unique_ptr<Comm>> comms;
  std::vector<std::unique_ptr<PcgDriver>> drivers;
  for (int r = 0; r < world; ++r) {
    solvers.push_back(std::make_unique<GpuSubdomainSolver>(spec, decompose_2d(spec.M, spec.N, pg, r), o));
    comms.push_back(make_recording_comm(&logs[size_t(r)], world, o.overlap));
    drivers.push_back(std::make_unique<PcgDriver>(std::vector<GpuSubdomainSolver*>{solvers.back().get()},
                                                  comms.back().get(), o.graph_batch));
  }
  // each rank's driver on its own (nothing is exchanged; the values are garbage, the call
  // sequence is what counts): init, then `iters` iterations -- captured when graph_batch > 0
  for (auto& d : drivers) {
    d->init();
    d->enqueue_iterations(iters);
    d->synchronize();
  }
  return logs;
}

int64_t max_square_grid(double bytes_per_gpu, int gpus, DType dtype, double reserve_fraction, int algo) {
  // pcg1 keeps 5 fields in either precision, the s-step PCG (fp64) 5 fields plus 2 fp64 face fields,
  // pcg2 4 fields; +1% pitch.  Auto (-1): the largest grid that fits SOME algorithm -- pcg1, to which
  // auto falls back when the s-step's fields do not fit (choose_algo)
  const double elem = dtype == DType::kFp64 ? 8.0 : 4.0;
  const double bpp = (algo == 3 ? 5.0 * elem + 16.0 : algo == 2 ? 4.0 * elem : 5.0 * elem) * 1.01;
  const double pts = bytes_per_gpu * (1.0 - reserve_fraction) * gpus / bpp;
  return int64_t(std::floor(std::sqrt(pts)));
}

}  // namespace pmx
