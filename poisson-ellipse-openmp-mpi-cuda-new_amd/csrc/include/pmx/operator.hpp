// The operator a launch runs -- plain, sigma, shift field, shift field plus face fields -- and the value rules of
// the user fields (rhs, w0, reaction, diffusion).  Host-only: no HIP header, so the CPU unit tests include it.
#pragma once

#include <cmath>
#include <cstdint>
#include <type_traits>
#include <utility>

#include "pmx/common.hpp"

namespace pmx {

// The values are the SH of k_init and k_apply.  k_pcg1 takes the pair (SH, DIF) below.
enum class OpKind : int { kPlain = 0, kSigma = 1, kField = 2, kDiffusion = 3 };
constexpr int pcg1_sh(OpKind k) { return int(k) < 2 ? int(k) : 2; }  // kShiftNone / kShiftSigma / kShiftField
constexpr bool pcg1_dif(OpKind k) { return k == OpKind::kDiffusion; }

// What defines A + shift on one subdomain: ProblemSpec::sigma; the shift field T(sigma + c) of a session with a
// reaction or a diffusion field; the face-coefficient fields ak, bk of a session with a diffusion field.  The
// fields at local (0, 0), in the storage type T (void: type-erased, as ApplyCoef keeps them).  A session with a
// level-set domain is a diffusion session (its face fields hold the domain's faces) that also keeps the
// right-hand-side mask: one byte per owned node, MemoryPlan::mask_bytes' layout.  The mask is no part of the
// operator -- only the inits read it.
template <typename T>
struct OperatorData {
  double sigma = 0.0;
  const T* shift = nullptr;
  const T* ka = nullptr;
  const T* kb = nullptr;
  const unsigned char* mask = nullptr;
  OpKind kind() const {
    if (ka) {
      PMX_CHECK(shift && kb, "a diffusion session holds the shift field and both face fields");
      return OpKind::kDiffusion;
    }
    if (shift) return OpKind::kField;
    return sigma != 0.0 ? OpKind::kSigma : OpKind::kPlain;
  }
};

// The four operator members of a kernel argument struct (InitData<T>, ApplyCoef) from the descriptor.  The mask is
// not among them: the inits copy it into InitData<T>::mask themselves.
template <typename X, typename T>
void set_operator(X& x, const OperatorData<T>& op) {
  x.sigma = op.sigma;
  x.shift = op.shift;
  x.ka = op.ka;
  x.kb = op.kb;
}

// f(std::integral_constant<OpKind, kind>{}): the one branch on the run-time kind
template <typename F>
decltype(auto) with_op_kind(OpKind kind, F&& f) {
  switch (kind) {
    case OpKind::kDiffusion: return f(std::integral_constant<OpKind, OpKind::kDiffusion>{});
    case OpKind::kField: return f(std::integral_constant<OpKind, OpKind::kField>{});
    case OpKind::kSigma: return f(std::integral_constant<OpKind, OpKind::kSigma>{});
    default: return f(std::integral_constant<OpKind, OpKind::kPlain>{});
  }
}

// Value rules of a global (M+1) x (N+1) fp64 field: rhs and w0 are finite on every node; a reaction field is
// finite and >= 0 on the interior nodes 1..M-1 x 1..N-1 (its box-boundary values are never read; -0.0 passes); a
// diffusion field is finite and > 0 on every node; a level-set field (domain) is finite on every node.
enum class FieldRule { kFinite, kNonNegInterior, kPositive };

// "<name>" + this: the refusal of a field that breaks its rule
inline const char* field_rule_text(FieldRule rule) {
  switch (rule) {
    case FieldRule::kNonNegInterior: return " must be finite and >= 0 on every interior node";
    case FieldRule::kPositive: return " must be finite and > 0 on every node";
    default: return " holds non-finite values";
  }
}

// host memory, row stride ld elements; reads the nodes the rule covers and nothing else
inline bool field_values_ok(const double* p, int64_t ld, int M, int N, FieldRule rule) {
  const int e = rule == FieldRule::kNonNegInterior ? 1 : 0;
  auto all = [&](auto ok) {
    for (int i = e; i <= M - e; ++i)
      for (int j = e; j <= N - e; ++j)
        if (!ok(p[int64_t(i) * ld + j])) return false;
    return true;
  };
  switch (rule) {
    case FieldRule::kNonNegInterior: return all([](double v) { return v >= 0.0 && !std::isinf(v); });
    case FieldRule::kPositive: return all([](double v) { return v > 0.0 && !std::isinf(v); });
    default: return all([](double v) { return std::isfinite(v); });
  }
}

}  // namespace pmx
