// Host-side launchers of the HIP kernels (csrc/hip/*.hip).
//
// Fused PCG iteration (redesigned to 2 streaming kernels / iteration):
//   pcg_a : p^k = D^-1 r + beta p^{k-1} on the tile + 1-cell ring (LDS row ring), A p^k on the
//           tile, block partial (A p^k, p^k)        [replaces K7 + K1 + K3(Ap,p) of the reference]
//   pcg_b : A p^k recomputed from p^k, w += alpha p, r -= alpha A p, z = D^-1 r (not stored),
//           block partials sum dw^2 and (z, r), halo pack of r  [replaces K6 + K2 + K3(z,r) + D1]
//   reduce: deterministic single-block finish of the block partials into the PcgState scalars.
// HBM traffic: 3 T/pt for pcg_a (r, p_old read, p write) + 5 T/pt for pcg_b (p, w, r read,
// w, r write) = 64 B/pt/iter in fp64 vs ~176 B/pt in the reference.
#pragma once

#include <hip/hip_runtime.h>

#include <vector>

#include "pmx/device_types.hpp"
#include "pmx/operator.hpp"

namespace pmx {

// One dispatch slot of a pcg1 order table: the tile, and the coefficient class (2 bits: 0 cut,
// 1 all faces inside D, 2 all outside) of each row r = 0..31 the tile's march visits, row r being
// local row i0 - 3 + r (the pipeline's initial row, then rows i0-2 .. i1+2).  With the classes in
// the slot a wave finds a row's class with a shift instead of ~11 scalar loads and ~20 compares.
struct Pcg1Slot {
  int id;
  int pad;
  unsigned long long cls;
};

struct TileCfg {
  int kind = 0;       // 0: workgroup tile + LDS row ring (pcg_kernels.hip)
                      // 1: wave tile + DPP lane shifts, software-pipelined register ring
                      // 2: wave tile + DPP lane shifts, ring-free short tiles (pcg_b only)
                      // 3: single-pass pcg1 tiles (overlapped by 2 columns, 3-stage row pipeline)
  int block = 256;    // columns per tile (kind 0: = threads per block; kind 1: = 64*vec)
  int rows = 0;       // rows per tile (marching length); 0 = auto
  int vec = 1;        // kind 1: columns per lane
  int waves = 1;      // kind 1: independent wave tiles per workgroup
  int abl = 0;        // kernel-isolation ablation bits (kAbl*), 0 in production
  int pair_w = 0;     // kind 2: paired w updates (k_pcg_b_rows_paired, pcg_kernels_dpp.hip)
  int pf = 1;         // kind 3: rows prefetched ahead of the computed row
  int tiles_i = 0, tiles_j = 0;
  // kind 3 on decomposed grids: the tiles [ti_lo, ti_hi) x [tj_lo, tj_hi) read no ghost cell of a
  // side that has a neighbour ("interior"); the rest form the frame (see launch_pcg1's part)
  int ti_lo = 0, ti_hi = 0, tj_lo = 0, tj_hi = 0;
  // kind 3: dispatch order of the whole-grid (order0) and interior (order1) launches: position
  // -> tile id, the tiles the ellipse cuts first within each XCD's share (pcg1_build_order);
  // nullptr = natural order
  const Pcg1Slot* order0 = nullptr;
  const Pcg1Slot* order1 = nullptr;
  const Pcg1Slot* order2 = nullptr;  // the frame tiles
  int groups[3] = {0, 0, 0};  // waves > 1: workgroups of each part (lockstep groups, pcg1_build_order)
  int arith32 = 0;  // kind 3 with fp32 storage: 1 = fp32 stencil arithmetic (GpuOptions::arith32)
  int lds_pad = 0;  // kind 3: dynamic LDS bytes per workgroup that cap the resident waves per CU
  int dpf = 0;      // kind 3: FAST tiles prefetch their rows dpf ahead by LDS-DMA (0 = registers)
  int bwaves = 8;   // kind 3 block tiles (pcg1_block.hip): waves per workgroup
  int interior_tiles() const { return (ti_hi - ti_lo) * (tj_hi - tj_lo); }
  int ntiles() const { return tiles_i * tiles_j; }
};

TileCfg make_tiles(const DevGeom& G, int block, int rows);
// rows = 0: auto, about target_tiles tiles but no taller than max_auto_rows
TileCfg make_wave_tiles(const DevGeom& G, int vec, int waves, int rows, int max_auto_rows = 32,
                        int target_tiles = 22000);
// kind 2 tiles for k_pcg_b_rows (rows = 0: 2)
TileCfg make_row_tiles(const DevGeom& G, int vec, int waves, int rows);
// kind 3 tiles for k_pcg1: 64*vec - 4 owned columns, rows = 0: auto
TileCfg make_pcg1_tiles(const DevGeom& G, int vec, int waves, int rows, int pf = 0, int elem = 8);
// padding LDS (bytes per workgroup) that lets at most wpcu workgroups of k_pcg1 (static LDS: 4 KiB
// per wave) share a CU; 0 for no cap
int pcg1_lds_pad(int wpcu, int waves);

enum ReduceMode : int { kSkipIfDone = 1, kBumpIter = 2 };

// Ablation bits for the kernel-isolation benchmark (GpuSubdomainSolver::bench_kernel): each
// switches off one part of the wave-tile kernels so its cost can be measured.  Results are
// numerically meaningless with any bit set.
enum AblBits : int {
  kAblHalo = 1, kAblAp = 2, kAblCoef = 4, kAblStore = 8,
  kAblHaloLoads = 16,  // skip the halo-column loads (k_pcg_a) / edge loads (k_pcg_b)
  kAblNoXcd = 64,      // identity workgroup -> tile mapping instead of the XCD-aware remap
};

template <typename T>
void launch_init(const DevGeom& G, const DevTables& Tb, T* w, T* r, HaloBufs<T> H,
                 double* partials, const TileCfg& tc, hipStream_t s,
                 const OperatorData<T>& op = {});  // op.kind() picks the kernel (as InitData's operator members)

// k_init with data (GpuSubdomainSolver::set_init_data / residual_norm), on launch_init's tiling.
//   data init (measure = false): r holds f on the owned nodes (has_f; else the constant G.F), w holds
//     w0 on the owned nodes and a 1-cell ring (has_w; else w0 = 0).  r <- T(B - A w0), B = f inside D
//     and 0 outside; the (z0, r0) partials and pcg2's packed r edges as launch_init.  w is only read.
//   measure: nothing is stored; partials[2 t + 1] = sum over tile t of (B - A w)^2, w with the
//     npend pending steps w + ca pa (+ cb pb) applied as launch_error_norms applies them; B from f
//     (element (i, j) at f[i * fpitch + j]; nullptr: G.F).  r and H are unused.
enum InitMode : int { kInitPlain = 0, kInitData = 1, kInitMeasure = 2 };
template <typename T>
struct InitData {
  const T* f = nullptr;
  int64_t fpitch = 0;  // data init: the fields' pitch (f is read from r)
  int has_f = 0, has_w = 0;
  const T* pa = nullptr;
  const T* pb = nullptr;
  double ca = 0.0, cb = 0.0;
  int npend = 0;
  // data init with has_w under the residual stop rule: partials[2 t] = sum over tile t of B^2 / D, the
  // rho_B = (D^-1 B, B) the tolerance is relative to (else that slot is 0, as in every other mode)
  int rho_b = 0;
  // screened problem (ProblemSpec::sigma): != 0 launches the kernels built for A + sigma I, D + sigma
  double sigma = 0.0;
  // a session with a reaction field: its shift field T(sigma + c) at local (0, 0), the fields' layout; non-null
  // launches the kernels that read the node's own shift instead of sigma
  const T* shift = nullptr;
  // a session with a diffusion field (it always holds a shift field too): its complete face-coefficient fields
  // ak(i, j) -- the face between nodes (i-1, j) and (i, j) -- and bk(i, j) -- between (i, j-1) and (i, j) --
  // at local (0, 0), the fields' layout; non-null launches the kernels that read the four faces of a node from
  // them instead of forming them from the 1-D tables
  const T* ka = nullptr;
  const T* kb = nullptr;
  // a session with a level-set domain (a diffusion session): its right-hand-side mask, one byte per owned node
  // -- node (i, j) at mask[(i - 1) pitch + j], != 0 inside D -- read in place of the ellipse predicate by the
  // diffusion kernels; null: the ellipse.  The last member: kernels built before it see their arguments where
  // they were.
  const unsigned char* mask = nullptr;
};
template <typename T>
void launch_init_data(const DevGeom& G, const DevTables& Tb, T* w, T* r, HaloBufs<T> H, double* partials,
                      const TileCfg& tc, const InitData<T>& X, bool measure, hipStream_t s);

// StopRule::kResidual: forms PcgState::rho_b / stop_thr2 from the init's reduced sums and tests rho_0
// (k_stop_init).  Enqueued once per init, after its reductions and all-reduces.
void launch_stop_init(PcgState* S, hipStream_t s);

template <typename T>
void launch_pcg_a_wave(const DevGeom& G, const DevTables& Tb, const T* r, T* p0, T* p1,
                       HaloBufs<T> H, double* partials, PcgState* S, const TileCfg& tc, bool exact,
                       hipStream_t s);
template <typename T>
void launch_pcg_b_wave(const DevGeom& G, const DevTables& Tb, T* w, T* r, const T* p0,
                       const T* p1, HaloBufs<T> H, double* partials, PcgState* S,
                       const TileCfg& tc, bool exact, hipStream_t s);

// Single-pass PCG iteration (pcg1_kernels.hip): p^k, A p^k, w, r^k, z^k, A z^k in one sweep,
// 5 partials per tile (rho, (Az,z), (Az,p), (Ap,p), |p|^2).  S->it == 0 is the init sweep.
// r is double-buffered (overlapped tiles read neighbour rows/columns of r^{k-1} while others
// write r^k): sweep k reads (k & 1 ? r2 : r).  Decomposed grids read the radius-2 ghosts that
// launch_pcg1_halo unpacked into the fields.
// part: 0 = every tile; 1 = the interior tiles only (they read no ghost cell, so they may run
// while the previous sweep's ghost exchange is still in flight); 2 = the frame tiles only.
// Parts 1 and 2 of one sweep may run concurrently on two streams: they write disjoint partials.
// wsweep: launch the kernel that moves w; it must be set exactly on the sweeps k >= 1 with
// k % S->w_cycle == 0 (the caller mirrors the device iteration counter; a mismatch stops the solve
// with status breakdown and the NaN flag).
// Builds tc.order0/order1/order2 in d_order (pcg1_order_slots(tc) slots): per launch part, the
// tiles of each XCD's share of the positions with their row classes; slow_first: the tiles with
// cut (slow-path) rows go first within each share.  Returns the number of such tiles.
// tc.waves > 1 (lockstep workgroups): the positions come in groups of tc.waves -- up to tc.waves
// adjacent tiles of ONE tile row, marched side by side by the waves of one workgroup; unused slots
// hold id -1; tc.groups[part] = the workgroups of each part, the XCD shares and the cut-first
// ordering are per group.
int pcg1_build_order(const DevGeom& G, const DevTables& Tb, TileCfg& tc, Pcg1Slot* d_order, bool slow_first,
                     hipStream_t s);
size_t pcg1_order_slots(const TileCfg& tc);  // d_order capacity pcg1_build_order needs

template <typename T>
void launch_pcg1(const DevGeom& G, const DevTables& Tb, T* w, T* r, T* r2, T* p0, T* p1,
                 double* partials, PcgState* S, const TileCfg& tc, hipStream_t s, int part = 0,
                 bool wsweep = false,
                 const OperatorData<T>& op = {});  // op.kind() picks the sigma, field or diffusion sweeps

// pcg1 sweep with block tiles (pcg1_block.hip): one workgroup per tc.rows x 124 tile, the three
// pipeline stages row-parallel; undecomposed fp64 grids; partial sums per tile as k_pcg1.  With a ticket the sweep also finishes the reduction (red_c =
// sums * weights, S->it + 1, progress[0]), replacing launch_reduce_n.
bool pcg1_block_shape_ok(int rows, int waves);  // an instantiated (rows, waves per workgroup) variant
template <typename T>
void launch_pcg1_block(const DevGeom& G, const DevTables& Tb, T* w, T* r, T* r2, T* p0, T* p1, double* partials,
                       PcgState* S, const TileCfg& tc, hipStream_t s, bool wsweep, const double* weights = nullptr,
                       unsigned* ticket = nullptr, long long* progress = nullptr);

// s-step PCG (ca_kernels.hip): s iterations per block of pass 1 (basis + Gram partials), one
// reduction that also runs the block's scalar recurrences, and pass 2 (p, z, w updated).
// Undecomposed fp64 grids; fields w and two (z, p) sets, the set read by a block in CaState::blk.
struct CaTiles {
  int s = 3;        // block size = basis degree (2 or 3)
  int he = 4;       // extra columns loaded per side ((s + 1) & ~1)
  int wo = 120;     // owned columns per wave tile (128 - 2 he)
  int rows = 0;     // rows per tile (pass 1)
  int tiles_i = 0, tiles_j = 0;
  int rows2 = 0, tiles_i2 = 0;  // pass 2's tile rows (same columns)
  int cwords = 0;   // row-class words per tile column (16 rows each)
  unsigned* tbl = nullptr;  // row classes (ca_build_classes), tiles_j * cwords words, owned by the caller
  const double* fa = nullptr;  // face coefficients a, b at every local node (ca_build_faces), pitched as
  const double* fb = nullptr;  // the fields, local (0, 0); read on the rows the ellipse cuts
  int gh = 2;                  // ghost rows of the fields on each side: 2, or 3 = s on a decomposed strip
  // pass 1's interior rectangle (every tile "fast": no Dirichlet node or partial width in reach):
  // [ti_lo, ti_hi) x [tj_lo, tj_hi); pass 2 runs every tile with one general kernel
  int ti_lo = 0, ti_hi = 0, tj_lo = 0, tj_hi = 0;
  int split = 1;       // pass 1: interior tiles by a fast-only kernel at 3 waves per SIMD, the frame by the general one
  int dma = 1;         // pass 1: interior tiles prefetch their rows by LDS-DMA (0: registers)
  // fused pass (k_ca_fused: pass 2 of block b + pass 1 of block b+1 in one march, radius 2s): its own
  // tiling of rows_f x wo_f (= 128 - 4 s) tiles, its interior rectangle and its row-class table
  int fuse = 0;
  int rows_f = 0, tiles_i_f = 0, tiles_j_f = 0, wo_f = 116, he_f = 6;
  int ti_lo_f = 0, ti_hi_f = 0, tj_lo_f = 0, tj_hi_f = 0;
  int split_f = 1;     // interior tiles by the fast-only kernel (launched first), the frame by the general one
  unsigned* tbl_f = nullptr;
  int ntiles() const { return tiles_i * tiles_j; }
  int ntiles2() const { return tiles_i2 * tiles_j; }
  int ntilesf() const { return tiles_i_f * tiles_j_f; }
};
// rows_f: the fused tiling's rows (0 = auto)
CaTiles make_ca_tiles(const DevGeom& G, int s, int rows, int rows2 = 0, int rows_f = 0);
int ca_nq(int s);  // partials per tile (pass 1's Gram products + pass 2's norms)
// fused: the classes of the fused tiling (t.he_f, t.wo_f, t.tiles_j_f columns) instead of pass 1/2's
void ca_build_classes(const DevGeom& G, const DevTables& Tb, const CaTiles& t, unsigned* tbl, hipStream_t s,
                      bool fused = false);
// fa / fb: local (0, 0) of two field-sized arrays (rows -1 .. nx+2 allocated)
void ca_build_faces(const DevGeom& G, const DevTables& Tb, double* fa, double* fb, int gh, hipStream_t s);
// the s-step's packed ghost exchange on 2-D blocks (k_ca_halo): pack z, p of one set into the send
// slots, or unpack the receive slots into the ghost rows / columns / corners
template <typename T>
void launch_ca_halo(const DevGeom& G, T* z, T* p, const HaloBufs<T>& H, int gh, bool unpack, hipStream_t s,
                    long long* progress);
// z = D^-1 r in place, p = z (the first block's set 0)
template <typename T>
void launch_ca_init(const DevGeom& G, const DevTables& Tb, T* z, T* p, hipStream_t s);
template <typename T>
// sframe: the stream of the frame tiles' kernel with t.split (nullptr: s); the caller forks and joins it.
// frame_wait: an event the tiles that read ghost rows wait for (the frame on sframe, or the whole pass)
void launch_ca_sweep(const DevGeom& G, const DevTables& Tb, T* w, T* z0, T* z1, T* p0, T* p1, double* partials,
                     const PcgState* S, const CaState* C, const CaTiles& t, bool upd, hipStream_t s,
                     hipStream_t sframe = nullptr, hipEvent_t frame_wait = nullptr);
// the fused pass (undecomposed grids, t.fuse): after the reduction of block b, block b's update and
// block b+1's Gram partials (the reduction then takes n = n2 = t.ntilesf()); a pending rewind instead
// rewinds w.  t.tbl_f: the fused tiling's row classes (ca_build_classes with fused = true).
template <typename T>
void launch_ca_fused(const DevGeom& G, T* w, T* z0, T* z1, T* p0, T* p1, double* partials, const CaState* C,
                     const CaTiles& t, hipStream_t s, hipStream_t sframe = nullptr, hipEvent_t frame_wait = nullptr);
// chunk: kCaReduceMaxBlocks * ca_nq(s) doubles of workspace; nmax: iterations this block may run
constexpr int kCaReduceMaxBlocks = 256;
// up to this many tiles the s-step reduction runs in one workgroup (k_ca_reduce1: no chunk hand-off)
constexpr int kCaReduce1Max = 12288;
// check_only: the pending stop test alone (after the last block of a batch; pass 2 then rewinds w if
// the test stopped inside that block)
// n / n2: pass 1 / pass 2 tiles (the partials of each)
// finish = false (decomposed grids): the rank's sums go to CaState::red for the all-reduce, and
// launch_ca_finish runs the scalars on the reduced sums afterwards
void launch_ca_reduce(const double* partials, int n, int n2, int s_, double h, double wdiff, int nmax,
                      bool check_only, PcgState* S, CaState* C, double* chunk, hipStream_t s,
                      long long* progress = nullptr, bool finish = true, bool residual = false);
// residual (both): the kernels built for StopRule::kResidual (ca_finish<S, true>), by ProblemSpec::stop
void launch_ca_finish(int s_, double h, double wdiff, int nmax, bool check_only, PcgState* S, CaState* C,
                      hipStream_t s, long long* progress = nullptr, bool residual = false);

// pcg1 ghost exchange: pack (unpack=false) the radius-2 edges of the buffers sweep `target` reads
// (parity of target) into H.send, or unpack H.recv into their ghost cells.
#ifdef PMX_WAVE_TRACE
void* pcg1_wave_trace_setup(long long it, int nwaves);
#endif

template <typename T>
void launch_pcg1_halo(const DevGeom& G, T* r, T* r2, T* p0, T* p1, HaloBufs<T> H, long long target,
                      bool unpack, hipStream_t s, long long* progress = nullptr);

// Halo/compute overlap: r^{k+1} on the subdomain edges that have a neighbour,
// written to the send buffers only, with exactly the arithmetic of pcg_b.  Runs first so the
// ghost exchange on the comm stream overlaps pcg_b, which then skips its own packing.
template <typename T>
void launch_edge_r(const DevGeom& G, const DevTables& Tb, const T* r, const T* p0, const T* p1,
                   HaloBufs<T> H, const PcgState* S, bool exact, hipStream_t s);

// Deterministic reduction of n block partials (nq interleaved values each) into out[0..nq),
// scaled by w0/w1.  `ws` is a per-solver workspace of kReduceWsDoubles doubles whose ticket
// word starts zeroed; the kernel re-arms it.  One workspace per stream (launches on a workspace
// must be stream-ordered).
constexpr int kReduceMaxBlocks = 64;
// k_reduce: chunk sums [0, 2*64) + ticket; k_reduce_n: its own chunk sums + ticket after that
constexpr int kReduceNOffset = 2 * kReduceMaxBlocks + 2;
constexpr int kReduceWsDoubles = kReduceNOffset + 8 * kReduceMaxBlocks + 2;
void launch_reduce(const double* partials, int n, int nq, double w0, double w1, double* out,
                   PcgState* S, int mode, double* ws, hipStream_t s);
// the same for nq = 5 interleaved values (k_pcg1 partials), out[q] = sum_q * weights[q].
// progress: optional host-mapped counters (GpuSubdomainSolver::progress): [0] <- S->it after the
// bump; launch_pcg1_halo counts [1] (exchanges packed) and [2] (exchanges unpacked).
void launch_reduce_n(const double* partials, int n, int nq, const double* weights, double* out,
                     PcgState* S, int mode, double* ws, hipStream_t s, long long* progress = nullptr);

// Deterministic in-process "all-reduce" across P subdomains on one device (LocalComm):
// out_k[q] = sum_r in_r[q] for every k, summed in rank order.
void launch_local_allreduce(double* const* bufs, int nranks, int nq, hipStream_t s);

// Per-row coefficient classes (see DevTables::acls); rows gi = 0..M+1, columns j = 0..N+1.
void launch_classify(const DevGeom& Gglobal, const DevTables& Tb, int* acls, int* bcls, hipStream_t s);

// MFMA wave reductions on test data: per wave64 w, out[3w..3w+2] = (sum x, sum x, sum x^2)
template <typename T>
void launch_wave_sums(const T* x, T* out, int nwaves, hipStream_t s);

// ---- unfused ops (tests, naive solver mode, bit-equality checks) ----
// All fields are local arrays with ghost ring: element (li,lj) at f[li*pitch+lj].
void launch_assemble(const DevGeom& G, const DevTables& Tb, double* a, double* b, double* B,
                     int64_t pitch_ab, hipStream_t s);
template <typename T>
void launch_apply_a(const DevGeom& G, const DevTables& Tb, const T* p, T* Ap, bool exact,
                    hipStream_t s);
template <typename T>
void launch_precond(const DevGeom& G, const DevTables& Tb, const T* r, T* z, bool exact,
                    hipStream_t s);
// partial sums of x*y over the interior into partials[nblocks]; returns nblocks used
template <typename T>
int launch_dot_partials(const DevGeom& G, const T* x, const T* y, double* partials, int max_blocks,
                        hipStream_t s);

// Error vs the analytic solution (k_error_norms): per block (sum e^2 in D, max |e| in D, max w)
// into out[3 * nblocks]; w_eff = w + ca pa (+ cb pb) for npend = 1 (2) pending w steps.  Returns
// the number of blocks used.
template <typename T>
int launch_error_norms(const DevGeom& G, const DevTables& Tb, const T* w, const T* pa, double ca,
                       const T* pb, double cb, int npend, double* out, int max_blocks, hipStream_t s);

// Device-resident user data (io_kernels.hip).  `src` / `out`: fp64 device arrays with row stride ld
// elements and unit column stride.
// rows x cols of src -> dst (row stride pitch), rounded to T as the host staging rounds
template <typename T>
void launch_scatter(const double* src, int64_t ld, T* dst, int64_t pitch, int rows, int cols, hipStream_t s);
// *flag <- 1 if a value of the global (M+1) x (N+1) array `field` breaks `rule` (the caller zeroes it first): one
// of k_finite, k_reaction_check and k_diffusion_check over the nodes field_values_ok reads
void launch_value_check(FieldRule rule, const double* field, int64_t ld, int M, int N, int* flag, hipStream_t s);
// A reaction field (io_kernels.hip).  launch_scatter with dst = T(sigma + src), rounded once
template <typename T>
void launch_scatter_shift(const double* src, int64_t ld, T* dst, int64_t pitch, int rows, int cols, double sigma,
                          hipStream_t s);
// A diffusion field (io_kernels.hip).  The face-coefficient fields of one subdomain from the nodal values
// k (global (M+1) x (N+1), row stride ld, device memory) and the 1-D tables:
//   ak(li, lj) = T((0.5 (k[gi-1, gj] + k[gi, gj])) a(gi, gj)),  bk(li, lj) = T((0.5 (k[gi, gj-1] + k[gi, gj])) b(gi, gj))
// in fp64, rounded once, with a / b the exact face formulas (coef_a / coef_b, as the s-step's face fields);
// faces that do not lie between two nodes of the box get 1.  ak, bk point to local (0, 0), row stride
// G.pitch; written: local rows -1 .. nx+3 of ak, -1 .. nx+2 of bk, columns -1 .. G.pitch-2 (the whole row).
template <typename T>
void launch_face_fields(const DevGeom& G, const DevTables& Tb, const double* k, int64_t ld, T* ak, T* bk, hipStream_t s);
// A level-set domain (io_kernels.hip).  The same two fields, on the same cells, with the geometric factor from
// the nodal level-set values phi (global (M+1) x (N+1), row stride ldp, device memory) instead of the tables --
// geo::ls_coef_a / ls_coef_b, each cell reading its 2 x 3 and 3 x 2 nodes of the global array, across
// subdomain borders -- and k optional (null: k = 1, the factor 0.5 (1 + 1) = 1 exactly).  mask (MemoryPlan::
// mask_bytes' layout): byte (li - 1) pitch + lj <- phi < 0 at the node, on the owned nodes.
template <typename T>
void launch_domain_fields(const DevGeom& G, const double* phi, int64_t ldp, const double* k, int64_t ld, T* ak, T* bk,
                          unsigned char* mask, hipStream_t s);
// local nodes (li0 .. li0+rows-1) x (lj0 .. lj0+cols-1) of a subdomain with local (0, 0) at global
// (gi0, gj0) -> out[gi * ld + gj]: w + ca pa (+ cb pb) as launch_error_norms forms it (w, pa, pb point to
// local (0, 0), row stride pitch); nodes on the global boundary (gi in {0, M}, gj in {0, N}) get zero
template <typename T>
void launch_gather(const T* w, const T* pa, double ca, const T* pb, double cb, int npend, int64_t pitch,
                   double* out, int64_t ld, int li0, int lj0, int rows, int cols, int gi0, int gj0, int M, int N,
                   hipStream_t s);

// The operator on device tensors (apply_kernels.hip).  Global rows gi_lo .. gi_lo + rows - 1 and columns
// gj_lo .. gj_lo + cols - 1 of out (row stride ldo) <- alpha (A + sigma I) x + beta x + gamma y + c0 on
// interior nodes, 0 on the box boundary; x, y (null: no y term; may be out), out are global (M+1) x (N+1)
// fp64 arrays with unit column stride, x read as 0 on the box boundary and never loaded there.  G supplies
// M, N and the mesh constants, Tb the global face tables; sigma != 0 launches the kernel built for it.
// plain: alpha = 1, beta = 0, no y, c0 = 0 -- (A + sigma I) x itself is stored.
struct ApplyCoef {
  double alpha = 1.0, beta = 0.0, gamma = 0.0, c0 = 0.0, sigma = 0.0;
  int plain = 1;
  // a session with a reaction field: the shift field T(sigma + c) of the subdomain that owns the block, at its
  // local (0, 0) -- global (sgi0, sgj0) -- with row pitch spitch and selem bytes per element; read in
  // sigma's place.  Null: sigma.
  const void* shift = nullptr;
  int64_t spitch = 0;
  int sgi0 = 0, sgj0 = 0, selem = 8;
  // a session with a diffusion field: the owning subdomain's face-coefficient fields (InitData::ka / kb), in
  // the shift field's layout and element type; read in place of the faces from the tables.  Null: the tables.
  const void* ka = nullptr;
  const void* kb = nullptr;
};
void launch_apply(const DevGeom& G, const DevTables& Tb, const double* x, int64_t ldx, const double* y, int64_t ldy,
                  double* out, int64_t ldo, int gi_lo, int gj_lo, int rows, int cols, const ApplyCoef& K,
                  hipStream_t s);

}  // namespace pmx
