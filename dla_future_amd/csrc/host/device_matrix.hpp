// device_matrix.hpp -- the Hermitian matrix of the Cholesky in device tile layout, its per-factorization workspaces,
// and the executor that issues the right-looking tile DAG onto HIP streams/events (device_matrix.cpp, cholesky.cpp).
//
// It stands where the reference has pika senders + async_rw_mutex tile pipelines
// (sender/transform.h:55-103, matrix/internal/tile_pipeline.h:36-51) and Panel workspaces (matrix/panel.h:42-631).
#pragma once
#include <atomic>
#include <cstddef>
#include <vector>

#include "distribution.hpp"
#include "runtime.hpp"
#include "transport.hpp"

namespace dlaf_mi355x {

// resident workgroups of the bulk update kernel on this GPU (CUs x blocks per CU)
template <class T>
long update_bulk_slots();

// ------------------------------------------------------------------------------------------------
// Device matrix in tile layout + the per-factorization workspaces.
template <class T>
struct DeviceMatrix : MatrixBase {
  Grid* grid = nullptr;
  char uplo = 'L';
  bool transposed = false;  // uplo == 'U': the device holds the transposed view, factored as lower
  Axis rows, cols;          // distribution of the VIEW
  long n = 0;
  int nb = 1;
  long nt = 0;
  long ltr = 0, ltc = 0;    // local tiles of the view
  size_t tile_elems = 0;    // nb*nb

  T* tiles = nullptr;       // ltr*ltc tiles
  T* diag_ws = nullptr;     // 2 x (nb*nb + ceil(nb/64)*64*64): received diagonal tile + its inverse blocks
  T* winv = nullptr;        // 2 x ceil(nb/64) * 64*64 inverted diagonal blocks (owner side)
  T* panel[2] = {nullptr, nullptr};   // ltr tiles each (received column panel)
  T* panelT[2] = {nullptr, nullptr};  // ltc tiles each (transposed panel)
  T* staging = nullptr;     // column-major staging for upload/download
  size_t staging_elems = 0;
  unsigned* coop_sync = nullptr;  // flags / counters: [update slices | one slice per diagonal tile], see the constructor
  size_t coop_sync_words = 0, coop_sync_update_slices = 0, coop_sync_potrf_words = 0;
  int* info = nullptr;      // device flag
  int* info_host = nullptr; // pinned

  hipStream_t s_high = nullptr, s_low = nullptr, s_comm = nullptr;
  // per step: panel solved, lookahead columns updated, diagonal tile ready, panels received, head tile
  // solved / received; ev_start / ev_done fence a factorization on the three streams
  std::vector<hipEvent_t> ev_panel, ev_high, ev_diag, ev_bcast, ev_head, ev_headb, ev_start, ev_done;

  // live timing of the launch classes with HIP events on the stream each class runs on
  // (kind 0: trailing bulk update, 1: lookahead-column update, 2: panel TRSM, 3: tile POTRF chain)
  struct ProfSlot {
    std::vector<hipEvent_t> start, stop;
    size_t used = 0;
    double flops = 0, bytes = 0;   // algorithmic, summed over the launches of the last run
    double ms = 0;                 // filled by wait()
    long launches = 0;
  };
  ProfSlot prof[4];
  long bulk_slots = 0;  // resident workgroups of the bulk update kernel on this GPU (CUs x blocks per CU)
  bool profiling = true;
  void prof_begin(int kind, hipStream_t s);
  void prof_end(int kind, hipStream_t s, double flops, double bytes);

  // Transposed panel of a step down the process columns (communication/broadcast_panel.h:125-210), ONE
  // broadcast per root process row: the local tile columns jl >= jl_n fall into `period` classes by the
  // process row that owns global tile row global_of(jl); class c = tiles jl_n + c, jl_n + c + period, ...
  // lands contiguously at dst + c * ts2 (the root packs its -- strided -- tiles there first).  a_base: column
  // panel, tile of local row il at a_base + (il - il_n) * tile_elems.  The tile of the last global row is
  // never a gemm operand and stays out (:186-191).  Returns the number of broadcasts issued.
  int bcast_transposed_panel(Transport* tr, CommAxis ax_col, const T* a_base, long il_n, long jl_n, T* dst,
                             hipStream_t s, int& period, long& ts2);

  T* tile(long il, long jl) const { return tiles + (size_t) (il + jl * ltr) * tile_elems; }
  size_t winv_elems() const { return (size_t) ((nb + kDiagBlock - 1) / kDiagBlock) * kDiagBlock * kDiagBlock; }

  void create(Grid* g, char uplo_, long n_, int nb_, int isrc, int jsrc);
  void destroy();
  ~DeviceMatrix() override { destroy(); }

  void upload(const T* host, long ld);     // caller's local column-major array -> tiles
  // tiles -> caller's array (uplo triangle only).  staging_is_current: the staging copy was filled by upload()
  // from this same array and the caller has not run since (saves re-staging the diagonal tiles)
  void download(T* host, long ld, bool staging_is_current = false);
  void copy_from(const DeviceMatrix<T>& other);
  // Checker (miniapp/miniapp_cholesky.cpp:408-443): `this` holds the ORIGINAL matrix and is overwritten
  // with A - L L^H on the uplo triangle; returns max|A - L L^H| and max|A| over the whole grid.
  void residual_of(DeviceMatrix<T>& factor, double* max_diff, double* max_a);
  int factorize();                         // blocking; returns LAPACK-style info
  // factorize() of a matrix that upload() just filled from `host`, with the download of every finished
  // tile column overlapped with the rest of the factorization (a helper thread follows ev_panel[k]); on
  // return `host` holds the factor.  The blocking host entry points (dlaf_p?potrf ...) use it.
  int factorize_and_download(T* host, long ld);
  std::atomic<long> panels_issued{-1};     // last step whose ev_panel has been recorded by factorize_async
  void factorize_async();                  // enqueue only
  // drain + info.  On a process grid the LAPACK info is made the same on every rank (MAX over the grid of
  // the device flags: every kernel that saw the failing diagonal tile stored the same index, the others 0;
  // the scheduling-failure code wins over everything) -- collective, like the factorization itself.
  int wait();
  int local_info = 0;  // this rank's own device status word of the last wait(), before the grid agreed on one
  // one tile of the device copy (global tile indices of the caller's matrix, not of the transposed view)
  // to / from a dense host array; returns false when this rank does not own the tile
  bool fetch_tile(long gi, long gj, T* host, long ld);
  // Measurement hook (bench.py): the panel TRSM of step 0 ALONE on the device -- on a copy of the factored first
  // tile column (local rows below the diagonal) with the factored diagonal tile, `reps` launches between two HIP
  // events.  In the factorization the panel solves run beside the bulk update on a few free workgroup slots, so
  // their in-situ durations say nothing about the kernel; this does.  One-process grids, after factorize().
  // Returns the average ms per launch; *flops / *bytes: algorithmic work of one launch.
  double trsm_profile(int reps, double* flops, double* bytes);
};

// Lower Cholesky of one kb x kb diagonal tile (ld) on stream s, with its ceil(kb/64) inverted 64 x 64 diagonal blocks in
// winv (cholesky.cpp).  sync: potrf_coop_sync_words(kb) words the caller has zeroed on the stream.
template <class T>
void potrf_tile(T* t, int ld, int kb, T* winv, int* info, int info_base, unsigned* sync, hipStream_t s);
// The two forms potrf_tile chooses between by DLAF_MI355X_POTRF: one cooperative launch (sync_is_zero / count_strips as
// in launch_potrf_coop; potrf_tile passes true, true), or diagonal block + TRSM + update launches per 64 columns.
template <class T>
void potrf_tile_coop(T* t, int ld, int kb, T* winv, int* info, int info_base, unsigned* sync, hipStream_t s,
                     bool sync_is_zero, bool count_strips);
template <class T>
void potrf_tile_chain(T* t, int ld, int kb, T* winv, int* info, int info_base, hipStream_t s);

}  // namespace dlaf_mi355x
