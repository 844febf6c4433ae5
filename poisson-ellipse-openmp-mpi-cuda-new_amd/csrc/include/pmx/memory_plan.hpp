// The device memory layout of one subdomain's fields, face fields and tables: the one place that
// decides it.  GpuSubdomainSolver allocates from a MemoryPlan and takes every field address from it;
// the size estimate (`pmx --plan`, choose_algo) evaluates the same type.  Host-only, no HIP.
#pragma once

#include <cstddef>
#include <cstdint>

#include "pmx/decomp.hpp"
#include "pmx/spec.hpp"

namespace pmx {

enum class DType : int { kFp64 = 0, kFp32 = 1 };

struct MemoryPlan {
  size_t elem = 8;         // bytes per field element
  size_t align = 32;       // 256 B in field elements
  int gh = 2;              // ghost rows of the fields on each side
  int64_t pitch = 0;       // row pitch (elements)
  size_t field_off = 0;    // element offset of local (0,0) inside a field
  size_t field_bytes = 0;  // one field: local rows 1-gh .. nx+gh
  int nfields = 4;         // w, r, p0, p1 (+ r2, the second r / z buffer of pcg1 and the s-step)
  size_t face_off = 0;     // s-step face-coefficient fields (a, b; fp64 in the fields' pitch): the element
  size_t face_bytes = 0;   // offset of local (0,0) and the bytes of one of the two (0: none)
  size_t table_bytes = 0;  // the 1D face tables and row classes (upload_tables)
  // The shift field of a session with a reaction field: T(sigma + c) per node, one more field of field_bytes
  // with r's pitch and ghost layers, behind the nfields iteration fields (index shift_field()).  0 without:
  // every other plan is what it was.
  int nshift = 0;
  // The face-coefficient fields of a session with a diffusion field: two more fields behind the shift field,
  // bk (index diff_field(1)) and then ak (diff_field(0)) -- ak last, because the x faces need one more row
  // than r's layout (local rows -1 .. nx+3: stage A of the march on ghost row nx+2 reads ak of row nx+3);
  // that row is diff_extra bytes behind the last field.  0 without: every other plan is what it was.
  int ndiff = 0;
  size_t diff_extra = 0;
  // The right-hand-side mask of a session with a level-set domain: one byte per node on the owned rows
  // 1 .. nx in the fields' pitch (node (li, lj) at byte (li - 1) pitch + lj), behind everything above.
  // 0 without: every other plan is what it was.
  size_t mask_bytes = 0;

  MemoryPlan() = default;
  // algo: 1 pcg1, 2 pcg2, 3 the s-step PCG (GpuOptions::algo); ghost_rows: 2, or the s-step's s / 2s on
  // decomposed grids -- rows, and columns on 2-D blocks
  MemoryPlan(const ProblemSpec& spec, const Subdomain& sd, DType dtype, int algo, int ghost_rows, bool shift = false,
             bool diffusion = false, bool mask = false)
      : elem(dtype == DType::kFp64 ? 8 : 4), align(256 / elem), gh(ghost_rows), nfields(algo == 1 || algo == 3 ? 5 : 4),
        nshift(shift || diffusion ? 1 : 0), ndiff(diffusion ? 2 : 0) {
    const auto round_up = [](size_t x, size_t a) { return (x + a - 1) / a * a; };
    const bool ca = algo == 3;
    // +8 columns of padding: vector loads of VEC <= 4 columns starting at <= ny+3 stay in the row, and the
    // last padding element of a row is column -1 of the next one.  s-step 2-D blocks: + 2 gh + 8, so that
    // the right ghost columns ny+1 .. ny+gh of a row and the left ones of the next row -- that row's
    // padding read as columns -gh .. -1 -- never overlap
    pitch = int64_t(round_up(size_t(sd.ny + 2 + 8 + (ca && sd.grid.Py > 1 ? 2 * gh + 8 : 0)), align));
    // element (li, lj) at base[li * pitch + lj]; base = allocation + (gh-1) rows + (align-1), so that
    // column 1 of every row starts 256-B aligned
    const size_t rows = size_t(sd.nx + 2 * gh) * size_t(pitch);
    field_off = size_t(gh - 1) * size_t(pitch) + align - 1;
    field_bytes = round_up((align - 1 + rows) * elem, 256);
    if (ca) {
      face_off = size_t(gh - 1) * size_t(pitch) + 31;
      face_bytes = round_up((31 + rows) * 8, 256);
    }
    if (ndiff) diff_extra = round_up(size_t(pitch) * elem, 256);
    if (mask) mask_bytes = round_up(size_t(pitch) * size_t(sd.nx), 256);
    table_bytes = (4 * size_t(spec.M + 2) + 4 * size_t(spec.N + 2)) * sizeof(double) +
                  8 * size_t(spec.M + 2) * sizeof(int);
  }

  size_t fields_total() const { return mask_off() + mask_bytes; }
  // byte offset of the mask (its row 1, column 0) from the start of the fields
  size_t mask_off() const { return size_t(nfields + nshift + ndiff) * field_bytes + diff_extra; }
  int shift_field() const { return nshift ? nfields : -1; }  // at()'s index of the shift field, -1: none
  // at()'s index of a face-coefficient field (f: 0 ak, 1 bk), -1: none
  int diff_field(int f) const { return ndiff ? nfields + nshift + (f == 0 ? 1 : 0) : -1; }
  size_t faces_total() const { return 2 * face_bytes; }
  size_t total() const { return fields_total() + faces_total() + table_bytes; }
  size_t row_bytes() const { return size_t(pitch) * elem; }
  // byte offset of local (li, lj) of field f (0 w, 1 r, 2 p0, 3 p1, 4 r2) from the start of the fields
  size_t at(int f, int64_t li = 0, int64_t lj = 0) const {
    return size_t(f) * field_bytes + size_t(int64_t(field_off) + li * pitch + lj) * elem;
  }
  // ... of face field f (0 a, 1 b) from the start of the face fields
  size_t face_at(int f, int64_t li = 0, int64_t lj = 0) const {
    return size_t(f) * face_bytes + size_t(int64_t(face_off) + li * pitch + lj) * 8;
  }
};

}  // namespace pmx
