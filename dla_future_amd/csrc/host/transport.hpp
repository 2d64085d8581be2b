// transport.hpp -- the process grid and the broadcasts along its rows and columns.  It stands where the reference has
// the MPI communicator grid (communication/communicator_grid.h:37-153).  Implementations: transport_host.cpp (host
// callbacks, the recording wrapper, and the grid's own functions), transport_rccl.cpp, transport_peer.cpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <memory>
#include <vector>

namespace dlaf_mi355x {

// ------------------------------------------------------------------------------------------------
// Transport: the broadcast primitive along a process row / column (communication/kernels/
// internal/broadcast.h:36-119 in the reference: MPI_Ibcast).  Two implementations:
//   * RCCL over xGMI: ncclBroadcast on device buffers, stream-ordered (the production path);
//   * host callbacks: device -> pinned host -> user callback -> device.  This is the analogue of
//     the reference's non-GPU-aware-MPI staging (sender/with_temporary_tile.h:87-204) and what the
//     gloo-based tests and single-GPU multi-process runs use.
enum class CommAxis : int { Row = 0, Col = 1 };

// root is the rank INSIDE the row/column communicator (= process column / row index)
typedef int (*dlaf_host_bcast_fn)(void* user, int axis, int root, void* host_buf, size_t bytes);
typedef int (*dlaf_host_barrier_fn)(void* user);

class Transport {
public:
  virtual ~Transport() = default;
  virtual bool device_side() const = 0;
  // device-side transports: enqueue on stream.  host-side: stream is synchronised first.
  virtual void bcast(CommAxis axis, int root, int my_index, const void* send, void* recv, size_t bytes,
                     hipStream_t stream) = 0;
  virtual void group_begin() {}
  virtual void group_end() {}
  virtual void barrier(hipStream_t stream) = 0;
  // max over every rank of the grid of n host doubles (the reference's sync::reduce with MPI_MAX in
  // max_norm, include/dlaf/auxiliary/norm/mc.h); result on every rank
  virtual void allreduce_max(double* host_vals, int n, int nprow, int npcol, int myrow, int mycol) = 0;
  // element-wise SUM of a device buffer over the ranks of a communicator, in place, result on every member
  // (the reference's schedule_all_reduce_in_place / schedule_reduce_* with MPI_SUM, communication/kernels/
  // all_reduce.h, reduce.h).  type: s, d, c, z; scope: 'A' the whole grid, 'R' my process row, 'C' my process column.
  // Every member ends up with the same bits (the host transport sums in root order, RCCL's ring does too).
  virtual void allreduce_sum(void* dev_buf, size_t count, char type, char scope, hipStream_t stream) = 0;
  // step marker of the executor (a no-op for real transports; the recording wrapper logs it)
  virtual void mark(long /*step*/) {}
  // the grid this transport serves (set by grid_transport)
  int nprow = 1, npcol = 1, myrow = 0, mycol = 0;
};

// One communication event as the recording transport logs it (dlaf_mi355x_grid_comm_log_*): what the
// reference's CommunicatorPipeline token serialises (sender/transform_mpi.h:60-75) -- every member of a
// communicator must issue the same sequence.
struct CommEvent {
  long kind;   // 0 row broadcast, 1 column broadcast, 2 step marker, 3 barrier, 4 allreduce
  long root;   // broadcast: root index inside the communicator; marker: step
  long bytes;
  long group;  // 1: issued inside group_begin / group_end
};

struct Grid {
  int nprow = 1, npcol = 1;
  int myrow = 0, mycol = 0;
  int rank = 0, nranks = 1;
  char order = 'R';
  std::unique_ptr<Transport> transport;  // null for a 1x1 grid (host grids: created lazily)
  dlaf_host_bcast_fn host_bcast = nullptr;
  dlaf_host_barrier_fn host_barrier = nullptr;
  void* host_user = nullptr;
  // called once when the grid is freed (dlaf_free_grid / dlaf_finalize): releases what the creator of a
  // host grid keeps alive for the callbacks (the MPI shim's communicators)
  void (*on_free)(void*) = nullptr;
  void* on_free_user = nullptr;
  // communication log (tests): when on, `transport` is wrapped by a recorder that appends here
  bool comm_log_on = false;
  std::vector<CommEvent> comm_log;
  ~Grid() {
    transport.reset();
    if (on_free)
      on_free(on_free_user);
  }
};

std::unique_ptr<Transport> make_rccl_transport(const void* unique_id, int nranks, int rank, int nprow,
                                               int npcol, int myrow, int mycol);
void rccl_get_unique_id(void* out128);
// creates the lazily-built host transport of a grid and, when the grid's communication log is on, wraps the
// transport with the recorder; idempotent.  Returns the transport (null for a 1x1 grid without communicators).
Transport* grid_transport(Grid& g);
// The opening of an entry that may communicate: initialises the runtime (idempotent), then grid_transport; a grid of
// more than one process without a transport is fatal.  Returns the transport (null on one process).
Transport* checked_transport(Grid& g);
// One status word for the whole grid from every rank's own (collective; a one-process grid returns `info`): the
// SMALLEST positive LAPACK index wins -- ranks that did not see the failing tile keep computing on the garbage it
// broadcast and may flag a later pivot of their own --, and the scheduling-failure code wins over everything.
int agree_on_info(Grid& g, int info);
std::unique_ptr<Transport> make_host_transport(dlaf_host_bcast_fn bcast, dlaf_host_barrier_fn barrier,
                                               void* user);
// host-driven peer copies (hipIpc mappings + interprocess events), control messages over the host callbacks
std::unique_ptr<Transport> make_peer_transport(dlaf_host_bcast_fn bcast, dlaf_host_barrier_fn barrier,
                                               void* user);
std::unique_ptr<Transport> make_callback_transport(dlaf_host_bcast_fn bcast, dlaf_host_barrier_fn barrier,
                                                   void* user);

// Communication self-test of a grid: every member of every row / column communicator broadcasts a
// coordinate-dependent pattern in turn (in place, out of place and grouped, the three forms the
// factorization issues), then barrier + max-allreduce.  Returns the number of mismatching checks.
int grid_selftest(Grid& g, size_t bytes);

}  // namespace dlaf_mi355x
