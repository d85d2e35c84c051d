/*
 * isph_hip.h -- C ABI of libisph_hip.so: the MI355X (gfx950) implementation of
 * implicit-sph's pressure-Poisson / Helmholtz inner loop.
 *
 * This is the drop-in boundary.  Everything above it (the SolverLin /
 * PrecondWrapper C++ classes in implicit-sph_amd/host/, a LAMMPS adapter, the
 * Python ctypes binding) talks to the GPU only through these entry points:
 * plain pointers and sizes, opaque handles, int return codes
 * (0 = LAMMPS_SUCCESS, -1 = LAMMPS_FAILURE, ref: macrodef.h:20-24), no
 * exceptions, no torch types.  The caller keeps ownership of every pointer it
 * passes; the library owns the device mirrors it creates.
 *
 * "ref:" citations are relative to /root/reference/IMPLICIT-SPH/ and name the
 * reference interface each entry point replaces.
 *
 * Pointer arguments marked [h|d] may be host or device pointers; the `on_device`
 * flag of the call says which (0 = host, the library stages the copy).
 * There is NO CPU fallback: every compute entry point fails with -1 if no
 * HIP device is usable.
 */
#ifndef ISPH_HIP_H
#define ISPH_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct isph_ctx isph_ctx;   /* device, stream, workspaces, RCCL communicator */
typedef struct isph_mat isph_mat;   /* device matrix: sliced-ELL (+ CSR view) + halo plan */
typedef struct isph_prec isph_prec; /* device preconditioner */

#define ISPH_SUCCESS 0
#define ISPH_FAILURE (-1)
#define ISPH_UID_BYTES 128

/* ---- context ---------------------------------------------------------- */

/* Replaces the Epetra_MpiComm every reference object is built on
 * (ref: solver_lin.cpp:30-31, precond.h:26).  `stream` = an existing
 * hipStream_t to launch on (NULL: the library creates its own). */
int isph_ctx_create(int device, void *stream, isph_ctx **ctx);
/* Multi-GPU: one process per GPU; the communicator is RCCL.  `uid` is the
 * ncclUniqueId (ISPH_UID_BYTES) produced on rank 0 by isph_comm_unique_id
 * and broadcast by the launcher (torch.distributed / MPI). */
int isph_comm_unique_id(char *uid);
int isph_ctx_create_dist(int device, void *stream, int rank, int nranks,
                         const char *uid, isph_ctx **ctx);
/* Multi-rank WITHOUT RCCL: ranks that share a device (several MPI ranks of a LAMMPS run on one GPU -- RCCL refuses two
 * ranks of a communicator on one device), or a launcher that wants its own MPI communicator to carry the traffic as
 * the reference does (Epetra_MpiComm, ref: solver_lin.cpp:30-31).  The library stages the device buffers through pinned
 * host memory and calls back; kernels, streams and their order are those of the RCCL path, only the host waits.
 *   exchange : for p in [0,npeers): send[send_off[p] .. send_off[p+1]) -> rank peer[p], recv[recv_off[p] .. recv_off[p+1])
 *              <- rank peer[p]; all messages posted together (MPI_Irecv/MPI_Isend/MPI_Waitall); a peer may be the rank
 *              itself.  Every rank calls it in the same order; a rank without peers does not call it.
 *   allreduce: in place over all ranks, op 0 = sum, 1 = max; called by every rank.
 * Both return 0 on success.  host/mpi_transport.h is the MPI implementation the C++ mirror uses. */
typedef struct {
  void *user;
  int (*exchange)(void *user, int npeers, const int *peer, const double *send, const long long *send_off,
                  double *recv, const long long *recv_off);
  int (*allreduce)(void *user, double *buf, int count, int op);
} isph_host_transport;
int isph_ctx_create_hostcomm(int device, void *stream, int rank, int nranks, const isph_host_transport *transport,
                             isph_ctx **ctx);
/* Physical identity of HIP device `device` as this process sees it: its PCI bus id ("0000:c1:00.0"), zero-padded to
 * ISPH_DEVICE_ID_BYTES.  Two ranks share a GPU exactly when their strings are equal -- their ordinals say nothing when
 * every rank runs under its own ROCR_VISIBLE_DEVICES mask (host/solver_lin_hip.h picks the transport by it). */
#define ISPH_DEVICE_ID_BYTES 64
int isph_device_identity(int device, char id[ISPH_DEVICE_ID_BYTES]);
int isph_ctx_sync(isph_ctx *ctx);
void isph_ctx_destroy(isph_ctx *ctx);
/* Device buffers released by the library are kept for the next set-up (the reference rebuilds matrix and preconditioner
 * every time step, pair_isph.cpp:1257-1287,1363) up to 80 % of the device's memory (a failed allocation trims them first).  isph_pool_trim() synchronises the
 * device and returns them to the driver; isph_pool_cached_bytes() reports how much is held.  No reference counterpart
 * (the reference has no device memory). */
int isph_pool_trim(void);
/* Upper limit of the cache in bytes (default: 80 % of the device memory that was free when the
 * library first gave a block back; bytes <= 0 restores the default).  A process that shares the
 * device with another allocator (torch, a second library) sets this to what it can spare, or calls
 * isph_pool_trim() before the other allocator needs the memory. */
int isph_pool_set_cap(long long bytes);
/* The triangular-solve stream of the block ILU / Gauss-Seidel set-up is reserved at twice a proven bound of its size
 * (one pass, no counting) unless that reservation exceeds this many bytes; above it the schedule first counts the
 * chunks of every block and the stream is allocated exactly (one more pass over the factor pattern, half the memory:
 * the smoother of the 4 M x 749 operator of BASELINE configs[4] takes 55 GB instead of 110).  Default 4 GiB;
 * bytes < 0 restores it, 0 sizes every stream exactly.  Process-wide.  No reference counterpart. */
int isph_set_exact_stream_threshold(long long bytes);
long long isph_pool_cached_bytes(void);
/* [0] bytes cached, [1] bytes handed out to live objects, [2] high-water mark of [1] (reset to [1] when reset_peak != 0),
 * [3] the cache limit in force (0: not yet determined). */
int isph_pool_info(long long info[4], int reset_peak);
const char *isph_last_error(void);

/* ---- matrix ----------------------------------------------------------- */

/* Ingress of an assembled local matrix: the three arrays
 * Epetra_CrsMatrix::ExtractCrsDataPointers returns after
 * FillComplete+OptimizeStorage (ref: pair_isph.cpp:1266-1270,
 * solver_lin.h:52 setMatrix).  Rows = locally owned particles; columns
 * [0,nrow) = owned, [nrow,ncol) = ghost columns filled by the halo exchange.
 * Replaces SolverLin::setMatrix / PrecondWrapper::setMatrix. */
int isph_mat_create_csr(isph_ctx *ctx, int nrow, int ncol, const int *rowptr /*[h|d]*/,
                        const int *colidx /*[h|d]*/, const double *val /*[h|d]*/,
                        int on_device, isph_mat **A);
/* The same ingress from HOST arrays, fused with the set-up of the block-Jacobi ILU(0)
 * preconditioner ("bjacobi-ilu0", block_size rows per subdomain): the matrix crosses PCIe in
 * chunks, and the set-up of the blocks whose rows have arrived runs while the rest is still on
 * the link.  What SolverLin_Belos::solveProblem does between receiving the host matrix and
 * starting Belos -- prec->create() = Ifpack Initialize + Compute (ref: solver_lin_belos.h:147-156,
 * precond_ifpack.h:60-74) -- with the result of isph_mat_create_csr(on_device = 0) followed by
 * isph_prec_create(A, "bjacobi-ilu0", block_size), bit for bit. */
int isph_mat_create_csr_bjacobi(isph_ctx *ctx, int nrow, int ncol, const int *rowptr /*[h]*/,
                                const int *colidx /*[h]*/, const double *val /*[h]*/, int block_size,
                                isph_mat **A, isph_prec **M);
/* The same with the caller's subdomains (see isph_prec_create_blocks): the result of isph_mat_create_csr(on_device = 0)
 * followed by isph_prec_create_blocks(A, nblocks, block_ptr), bit for bit. */
int isph_mat_create_csr_blocks(isph_ctx *ctx, int nrow, int ncol, const int *rowptr /*[h]*/, const int *colidx /*[h]*/,
                               const double *val /*[h]*/, int nblocks, const int *block_ptr /*[h]*/, isph_mat **A,
                               isph_prec **M);
/* The same ingress INTO THE LIBRARY'S OWN ROW NUMBERING (isph_ctx_set_ordering), for the drop-in path, where the matrix
 * arrives assembled in LAMMPS' atom order and no particle array comes with it: the caller hands over the coordinates of
 * its rows the way PrecondWrapper_ML::setCoordinates receives them (ref: precond_ml.h:63-94 -- three host arrays of nrow
 * doubles cut from atom->x, pair_isph.cpp:1290-1303; z may be NULL when dim == 2).  The rows are sorted into the bricks
 * of order.hpp from the coordinates, the matrix crosses the link as it is and is permuted on the device in one pass
 * (rows, owned columns, column order inside the rows).  The result behaves like a matrix from isph_assemble_poisson:
 * every vector at this boundary stays in the caller's numbering, isph_prec_create(.., block_size 0) uses the bricks. */
int isph_mat_create_csr_coords(isph_ctx *ctx, int nrow, int ncol, const int *rowptr /*[h]*/, const int *colidx /*[h]*/,
                               const double *val /*[h]*/, int dim, const double *x /*[h]*/, const double *y /*[h]*/,
                               const double *z /*[h]*/, isph_mat **A);
/* The same fused with the set-up of "bjacobi-ilu0" on the library's bricks: the staging threads gather the caller's rows
 * in the NEW order (the permutation is known before the first entry leaves the host), the conversion kernel renames the
 * columns and a ranged row sort follows it, so that -- as in isph_mat_create_csr_blocks -- the 16-bit column windows and
 * the ILU(0) extraction / schedule / factorisation of the bricks whose rows have arrived run while the rest of the matrix
 * is still on the link.  Result: the matrix of isph_mat_create_csr_coords and isph_prec_create(A, "bjacobi-ilu0", 0). */
int isph_mat_create_csr_coords_bjacobi(isph_ctx *ctx, int nrow, int ncol, const int *rowptr /*[h]*/, const int *colidx /*[h]*/,
                                       const double *val /*[h]*/, int dim, const double *x /*[h]*/, const double *y /*[h]*/,
                                       const double *z /*[h]*/, isph_mat **A, isph_prec **M);
/* Diagnostics of the last host-side ingress on this context (milliseconds since its start):
 * [0] staging threads started, device buffers reserved  [1] all chunks queued on the copy stream
 * [2] copy stream drained  [3] compute stream drained (conversion + fused set-up)  [4] end
 * [5] time the queueing thread waited for staged chunks  [6] bytes that crossed the link (16-bit
 * column differences where the rows allow them: 10 instead of 12 per entry)  [7] staging threads.
 * No reference counterpart. */
int isph_ingress_info(const isph_ctx *ctx, double info[8]);
/* KEEPING A MATRIX' PATTERN.  Within one time step the reference refills ONE Epetra matrix -- one graph -- with new values
 * and solves it several times (ref: pair_isph.cpp:1266-1270 allocates A.crs; :589 :636 :812 :925 :988-1011 refill it);
 * Epetra's ReplaceMyValues keeps the graph, and Ifpack's Compute() may be called again after one Initialize().
 * While isph_ctx_hold_pattern(ctx, 1) is in force, a matrix created from a CSR -- isph_mat_create_csr (host or device
 * arrays), _bjacobi, _blocks, _coords, _coords_bjacobi -- also keeps an ENTRY MAP: a device array that gives, for every
 * entry of the caller's CSR in the caller's entry order, its position in the sliced-ELL image (32 bits per entry, built on
 * the device from the image the ingress leaves there).  The map goes through whatever the ingress did to the entry: the
 * row sort of unsorted rows, and on the _coords routes the library's row permutation, the column renaming and the sort
 * by the new column.  The matrix owns its map; switching the mode off only affects later creations.  A matrix with a row
 * that holds the same column twice is created as without the mode, without a map.  Off by default: every call is then
 * what it was, launch for launch, and no map is reserved.
 * While the mode is on, an ILU(k > 0) created by isph_prec_create* also keeps the fill level of its entries (1 B per factor
 * entry), which isph_prec_refactor needs.  No reference counterpart as a call (Epetra keeps its graph by construction). */
int isph_ctx_hold_pattern(isph_ctx *ctx, int on);
/* New values for a matrix that carries a map: val holds nnz doubles in the entry order of the arrays A was created from.
 * Afterwards A is bit for bit the matrix a fresh create of the same route gives from (same rowptr, same colidx, val) --
 * the values are moved, not computed with; padding stays 0; row numbering, halo plan, 16-bit column windows and slice
 * offsets are untouched.  Host values travel through the pinned ring and the staging threads of the ingress in its chunks,
 * one copy per chunk, 8 B per entry on the link, with the scatter of a chunk queued behind its copy; device values take
 * one scatter launch.  isph_ingress_info then reports this call ([6] = 8 nnz).  Fails WITHOUT touching A when A has no
 * map or val is NULL.  Preconditioners built from A before the call are stale: a block ILU, a Chebyshev polynomial (its
 * float plane included) and an SA-AMG hierarchy created while the mode was on can be refreshed by isph_prec_refactor; every
 * other one must be rebuilt by the caller.
 * Replaces Epetra_CrsMatrix::ReplaceMyValues on a FillComplete'd matrix. */
int isph_mat_update_values(isph_ctx *ctx, isph_mat *A, const double *val /*[h|d]*/, int on_device);
/* [0] 1 when A carries a map  [1] bytes of the map  [2] value updates A has taken */
int isph_mat_pattern_info(const isph_mat *A, long long info[3]);
/* Halo plan = what Epetra builds inside FillComplete (column map + Import,
 * ref: functor_graph.h:97).  For peer p: send x[send_idx[send_ptr[p]..send_ptr[p+1])]
 * and receive the ghost columns nrow+recv_ptr[p] .. nrow+recv_ptr[p+1]. */
int isph_mat_set_halo(isph_ctx *ctx, isph_mat *A, int npeers, const int *peer_rank,
                      const int *send_ptr, const int *send_idx, const int *recv_ptr);
/* The same plan as a stand-alone object, for per-atom fields that are not matrix columns yet: LAMMPS'
 * comm->forward_comm_pair(this) with PairISPH::pack_forward_comm / unpack_forward_comm (ref: pair_isph.cpp:1924-2110;
 * call sites functor_volume.h:78-80 for Vfrac, pair_isph.cpp:977-979 Vstar, :1017-1019 DeltaP, :1123-1125 Pressure,
 * :1161-1163 Velocity).  isph_halo_forward sends ncomp doubles per listed owned atom (x is [nlocal][ncomp], the layout
 * of atom->v / the pair's per-atom arrays) and returns the ghost values in ghost-column order: ghosts is
 * [recv_ptr[npeers]][ncomp].  Runs on the context's stream over its RCCL communicator (grouped ncclSend/ncclRecv). */
typedef struct isph_halo_plan isph_halo_plan;
int isph_halo_create(isph_ctx *ctx, int nlocal, int npeers, const int *peer_rank, const int *send_ptr,
                     const int *send_idx, const int *recv_ptr, isph_halo_plan **plan);
int isph_halo_forward(isph_ctx *ctx, const isph_halo_plan *plan, const double *x /*[h|d]*/, double *ghosts /*[h|d]*/,
                      int ncomp, int on_device);
void isph_halo_destroy(isph_halo_plan *plan);
/* sizes: [0]=nrow [1]=ncol [2]=nnz [3]=number of 64-row slices
 *        [4]=stored (padded) entries [5]=bytes of the sliced-ELL arrays */
int isph_mat_info(const isph_mat *A, long long info[6]);
/* Export as CSR with sorted columns (device->host); caller sizes from info. */
int isph_mat_export_csr(isph_ctx *ctx, const isph_mat *A, int *rowptr, int *colidx, double *val);
/* Rows [row_begin, row_begin + nrows) as CSR, row pointers relative to the range (64-bit), columns ascending; fails
 * when the rows hold more than `capacity` entries.  For host-side checks of matrices beyond a 32-bit CSR (the
 * 3*10^9-entry operator of BASELINE configs[4]): a test exports a few thousand sampled rows and multiplies them itself.
 * No reference counterpart (Epetra_CrsMatrix::ExtractMyRowView is the closest). */
int isph_mat_export_rows(isph_ctx *ctx, const isph_mat *A, int row_begin, int nrows, long long *rowptr, int *colidx,
                         double *val, long long capacity);
/* *bits = 16 when the product of this matrix reads the windowed 16-bit copy of its columns (every 64-row slice touches at
 * most 64 aligned windows of 1024 columns, padding included), 32 when it reads the 32-bit columns (some slice touches more,
 * or the matrix is one of the library's own transfer / coarse operators).  Asks exactly as the product does, so the
 * 16-bit copy is built on the first call if no product has built it yet.  No reference counterpart. */
int isph_mat_column_bits(isph_ctx *ctx, const isph_mat *A, int *bits);
void isph_mat_destroy(isph_mat *A);

/* y = A x  (Epetra_CrsMatrix::Apply incl. the ghost Import; ref: solver_lin.h:133).
 * x: nrow owned entries -- the ghost columns are fetched through the halo plan; a matrix WITH ghost columns (ncol >
 * nrow) but WITHOUT a plan (isph_mat_set_halo not called) reads all ncol entries from the caller.  y: nrow entries. */
int isph_spmv(isph_ctx *ctx, const isph_mat *A, const double *x /*[h|d]*/,
              double *y /*[h|d]*/, int on_device);
/* Time `reps` back-to-back SpMV launches with HIP events on the library
 * stream; returns the average kernel time in milliseconds.  variant 0 = the production kernel; 1..6 = experimental
 * instantiations of the 32-bit-column kernel (unroll / cache policy), for scripts/spmv_variants.py only. */
int isph_spmv_time(isph_ctx *ctx, const isph_mat *A, const double *x_dev, double *y_dev,
                   int reps, int variant, double *avg_ms);

/* ---- preconditioner --------------------------------------------------- */

/* Replaces PrecondWrapper_Ifpack::create() = Ifpack factory + Initialize +
 * Compute (ref: precond_ifpack.h:52-75).  type:
 *   "none"          identity
 *   "jacobi"        point Jacobi (debug)
 *   "bjacobi-ilu<k>"  k = 0..8: block-Jacobi, ILU(k) per block == Ifpack
 *                   AdditiveSchwarz<ILU>, "Overlap Level"=0,
 *                   "fact: level-of-fill"=k (precond_ifpack.h:35; the reference's
 *                   default is k = 1), one block per `block_size` rows
 *                   (k > 0: block_size <= 1024 and the symbolic phase runs on the device)
 *   "bjacobi-ilu<k>-f32"  the same with value_bits = 32 (isph_ilu_params): the triangular solves stream the strict-L and
 *                   strict-U factor values rounded to single precision
 *   "ilu<k>"        ILU(k) of the whole local matrix: Ifpack on one MPI rank (precond_ifpack.h:60-74 with
 *                   Comm.NumProc() == 1); see isph_prec_create_schwarz
 *   "sa-amg"        PrecondWrapper_ML::create() with its default parameters and no null vector
 *                   (isph_prec_create_amg takes the parameters and the null vector of a singular system)
 *   "sa-amg-ilu<k>" k = 0..8: the same with ML's IFPACK smoother, block ILU(k) (isph_amg_params::smoother = 4,
 *                   ilu_fill = k; sph-script/ml-ifpack.xml asks for k = 4 and 3 sweeps)
 *   "chebyshev<d>"  d = 1..16: Chebyshev polynomial of degree d in D^-1 A, Ifpack's "Precond Type" = "Chebyshev"
 *                   (isph_prec_create_chebyshev takes the ratio and the eigenvalues)
 *   "chebyshev<d>-f32"  the same with value_bits = 32: the polynomial of A rounded to single precision
 *   "gmres-poly<d>" d = 1..25: Belos' GMRES polynomial of degree d in D^-1 A as a fixed preconditioner, without a null
 *                   vector (isph_prec_create_gmres_poly takes one; there is no "-f32" form)
 * Rebuilt every solve in the reference (solver_lin_belos.h:153,190). */
/* block_size 0 ("bjacobi-ilu<k>" only): the matrix' own subdomains, i.e. the bricks the assembly sorted the particles
 * into (isph_ctx_set_ordering); fails for a matrix in the caller's numbering. */
int isph_prec_create(isph_ctx *ctx, const isph_mat *A, const char *type, int block_size,
                     isph_prec **M);
/* "bjacobi-ilu0" on the CALLER'S subdomains: block b = rows block_ptr[b] .. block_ptr[b+1] (host array of nblocks + 1
 * ascending offsets from 0 to nrow, at most 1024 rows each; the rows of a subdomain are consecutive in the matrix).  The
 * reference's subdomains are the bricks of LAMMPS' spatial decomposition (one per MPI rank, ref: precond_ifpack.h:60-74
 * with pair_isph.cpp:1258-1259); a caller that numbers its particles brick by brick hands the brick boundaries over
 * here instead of accepting a cut every block_size rows -- a thin remainder brick at the edge of the box is then a
 * subdomain of its own shape and not the two halves of its neighbours.  Same kernels and data layout as
 * isph_prec_create("bjacobi-ilu0"). */
int isph_prec_create_blocks(isph_ctx *ctx, const isph_mat *A, int nblocks, const int *block_ptr, isph_prec **M);
/* The same with "fact: level-of-fill" = level_of_fill in 0..8 (ref: precond_ifpack.h:35, the reference's default is 1): the
 * level-of-fill pattern of every subdomain (Ifpack_IlukGraph's rule) is formed on the device by level_of_fill sweeps of
 * the merge kernel, whatever the lengths of the subdomains. */
int isph_prec_create_blocks_fill(isph_ctx *ctx, const isph_mat *A, int nblocks, const int *block_ptr, int level_of_fill,
                                 isph_prec **M);
/* The block stream ("bjacobi-ilu<k>") with all its parameters in one struct: level_of_fill 0..8, and one of the three
 * routes -- nblocks > 0: the caller's table block_ptr[0 .. nblocks] (isph_prec_create_blocks_fill); otherwise
 * block_size > 0: one block per block_size rows, block_size 0: the matrix' own subdomains (isph_prec_create).  With
 * value_bits 64 the call IS those calls, bit for bit.
 * value_bits (not a reference parameter): 64 (the default; 0 means the same) or 32; any other value is refused.  With 32
 * the factorisation is untouched -- isph_prec_export_ilu returns the fp64 factor bit for bit as value_bits 64 builds it --
 * and one more streaming pass behind it rounds the values of the triangular-solve stream to the nearest float (ties to
 * even, subnormals kept, a value that rounds to 0 accepted) into a plane of 4 B per entry; the fp64 stream is then given
 * back.  The application is exactly the fp64 triangular solves z = U^-1 D^-1 L^-1 r with every strict-L and strict-U
 * entry replaced by its float rounding: the pivots 1/d_i, the vectors (in LDS), the accumulators, the segmented scan and
 * the update stay double, the operations and their order are those of value_bits 64.  The solves stream 6 B instead of
 * 10 B per stream entry.  A fixed linear operator, so every Krylov solver may use it and the outer iteration works in
 * fp64 on the true A; but it is symmetric only up to single-precision rounding when A is symmetric, because
 * fl32(u_ij) != d_i fl32(l_ji) in general: "Block CG" sees a preconditioner that is nonsymmetric at the 1e-7 level.
 * The create call fails when a finite factor value exceeds the range of single precision.  isph_prec_value_bits
 * answers 32.  Off by default.
 * Measured at 100^3 on the library's bricks, widths alternated in one process (profiles/ilu_f32_100cubed.txt,
 * 2026-10-18): one application 127.9 (125.4 - 134.7) against 146.4 (144.6 - 149.0) us for 0.615 of the bytes ("bjacobi-
 * ilu0"), 299.0 (293.1 - 326.2) against 331.2 (326.6 - 344.0) us for 0.607 ("bjacobi-ilu1") -- time 0.87 and 0.90: the
 * solve is bound by its per-block dependency chain, not by the stream bytes; create + solve with the benchmark's
 * protocol 37.00 against 38.02 ms (71 iterations both) and 99.47 against 100.93 ms (63 both); the rounding pass +0.03 ..
 * +0.3 ms per create.
 * Call isph_ilu_params_default FIRST and then change fields: the struct grows at its tail. */
typedef struct {
  int level_of_fill;    /* 0..8 */
  int block_size;       /* rows per block; 0 = the matrix' own subdomains */
  int nblocks;          /* > 0: the caller's table */
  const int *block_ptr;
  int value_bits;       /* 64 (default; 0 means the same) or 32 */
} isph_ilu_params;
void isph_ilu_params_default(isph_ilu_params *p);
int isph_prec_create_ilu(isph_ctx *ctx, const isph_mat *A, const isph_ilu_params *prm, isph_prec **M);
/* Numeric refactorisation of a block-stream ILU ("bjacobi-ilu<k>", k = 0..8, every subdomain route and both value_bits of
 * isph_ilu_params, preconditioners returned by the fused ingress calls included) on the new values of A: Ifpack's
 * Compute() after one Initialize() (ref: precond_ifpack.h:60-74 runs both per solve).  KEPT: the row layout of the factor,
 * its columns and diagonal slots, the levels, the triangular-solve schedule (words, step bytes, row order) and the block
 * offsets.  REDONE: one kernel refills the factor values from the in-block entries of A's rows (ILU(k): merged into the
 * factor row, fill slots 0), then the factorisation kernel of the create call runs as it is (value_bits 32: the fp64 stream
 * is reserved again first, and the rounding pass and its release follow).  BIT FOR BIT what a fresh isph_prec_create_ilu on
 * A gives: isph_prec_export_ilu, the pivots, the stream, isph_prec_info and the application.  REFUSED: a row whose
 * in-block columns are not exactly the level-0 columns of its factor row (the message names the first such row), another
 * row count or subdomain table -- M is then valid only for isph_prec_destroy or another isph_prec_refactor; every other
 * preconditioner type (the message names it); an ILU(k > 0) created while isph_ctx_hold_pattern was off (its fill levels
 * were not kept).  A zero pivot shows exactly as after the create call.
 *
 * "chebyshev<d>" (isph_prec_create_chebyshev or isph_prec_create; both value_bits, both eig_type) CREATED WHILE
 * isph_ctx_hold_pattern WAS ON.  Nothing of the pattern is kept: the diagonal, rho or the estimate, the scalars and the
 * float plane are made again by the set-up of the create call with the parameters of the create call, so the application
 * is bit for bit that of a fresh create on A.  M applies A from then on (the caller keeps it alive).  REFUSED: another row
 * count; a polynomial created with the mode off (as before this type could be refactored: the mode is the caller's
 * statement that its preconditioners are meant to follow the matrix), M then untouched and usable.
 *
 * "gmres-poly<d>" (isph_prec_create_gmres_poly or isph_prec_create) CREATED WHILE isph_ctx_hold_pattern WAS ON: the same rule.
 * The diagonal, the Arnoldi steps, the roots and the steps of the application are made again with the degree and the
 * (normalised) null vector of the create call: bit for bit a fresh create on A.  REFUSED: another row count, a polynomial
 * created with the mode off, a null vector kept in another row numbering than A's; M then untouched and usable.
 *
 * "sa-amg" (isph_prec_create_amg or isph_prec_create; every smoother, cheb_value_bits, cycle_bits, eig_type, threshold,
 * with or without a null vector), on one rank, for a hierarchy CREATED WHILE isph_ctx_hold_pattern WAS ON -- ML's
 * MultiLevelPreconditioner::ReComputePreconditioner.
 *   KEPT: the aggregates of every level and the number of levels; the patterns of P_l, R_l = P_l^T, A_l P_l and A_{l+1};
 *   the transposition order; the SELL images of P_l, A_l P_l and A_{l+1} with their column windows; the layouts of the
 *   smoothers; the values of isph_prec_amg_path.
 *   REDONE on the values of A: the diagonal and rho of every level (eig_type 1: each level's estimate); the tentative
 *   prolongator on the kept member lists of the aggregates; the damping and the values of P_l, R_l, A_l P_l and A_{l+1}
 *   and of their SELL images; the smoothers (Chebyshev: the set-up again; dense 64-row blocks: built again; the ILU(k)
 *   streams of smoother 4: refactored in place as above; the Gauss-Seidel stream of the fine level: created again -- a
 *   value-only refill of it does not exist yet); the float planes of cheb_value_bits / cycle_bits = 32; the dense coarse
 *   inverse (a singular one is refused as in create).  The fine level points at A from then on: the caller keeps A alive.
 *   WHAT IT IS: the hierarchy of the new values ON THE KEPT AGGREGATES (ML's reuse semantics).  The second pass of the
 *   aggregation joins a leftover row to its most strongly coupled neighbour, so a fresh create on the new values may
 *   aggregate differently; where it aggregates the same, the refresh equals the fresh create to round-off (not to the
 *   bit: the sums run in another order).  Scaling the off-diagonal entries by one factor keeps their order and the diagonal
 *   never enters that pass: Newton Jacobians that change on the diagonal and the Helmholtz theta dt variants are such cases.
 *   A matrix whose pattern differs but whose terms all find a slot in the kept patterns gives a valid hierarchy of the kept
 *   aggregates (slots no term reaches hold 0).  Two refreshes from the same values give the same bits: every slot is
 *   summed in an order fixed by the data, without floating-point atomics (the create call does not promise this).
 *   The null vector of the create call stays; isph_prec_amg_set_nullvec replaces its values before a refactor.
 *   REFUSED, by name, M then valid only for isph_prec_destroy or another isph_prec_refactor: a hierarchy "created while
 *   the pattern was not held"; another row count or row numbering; a matrix with a halo or a context of more than one
 *   rank ("the neighbours' P rows would have to travel again: rebuild"); a term of P_l, A_l P_l or P_l^T A_l P_l that
 *   finds no slot in the kept pattern (the message names the level and the first such row).
 *   What the hold mode keeps per level on top of a plain create: the member list of the aggregates (8 B per row), the
 *   pattern of A_l P_l (8 B per row + 4 B per entry), the transposition map (4 B per entry of P_l) and the CSR of every
 *   coarse operator in the row order of its SELL image.  With the mode off the create call is what it was, launch for launch.
 *   ISPH_AMG_REFRESH_TWO_PASS=1 (read by the call): the values come from the count + fill passes of the two-pass kernels of
 *   the create call instead of the refresh kernels -- their cross-check and the baseline of their timing. */
int isph_prec_refactor(isph_ctx *ctx, isph_prec *M, const isph_mat *A);
/* Ifpack_AdditiveSchwarz<Ifpack_ILU> with the parameters PrecondWrapper_Ifpack sets (ref: precond_ifpack.h:30-45,
 * 60-74): "fact: level-of-fill" (default 1), "Overlap Level" (default 1), "schwarz: combine mode" (default "Add" = 0;
 * 1 = "Zero", restricted additive Schwarz).  block_size = 0: one subdomain = the whole local matrix, which is what
 * the reference factors on one MPI rank (Ifpack ignores the overlap there); block_size = B > 0: consecutive
 * subdomains of B rows (any B), each extended by `overlap` layers of the rows its columns reference, like the ranks
 * of a parallel run.  isph_prec_create(type = "ilu<k>") is the block_size = 0 case.  Level-scheduled on the device:
 * the fidelity path; "bjacobi-ilu<k>" is the throughput path.
 * info: [0] extended rows [1] factor entries [2] subdomains [3] L levels [4] U levels [5] longest factor row
 * [6] 2 = one workgroup per subdomain does both sweeps (many small subdomains), 1 = persistent launches, 0 = one launch
 * per dependency level (see level_launches).
 * export: rows[nloc] (global row of every local row), loc_ptr[nsub+1], factor CSR in local numbering. */
typedef struct {
  int level_of_fill, overlap, combine, block_size;
  int level_launches; /* 0 (default): the form is picked by the shape of the problem -- >= 32 subdomains of <= 4096 rows:
                         ONE launch per application, a workgroup per subdomain with its part of the vector in LDS and a
                         barrier per level; narrow levels (whole-matrix factors): the factorisation and every triangular
                         sweep are ONE persistent launch whose rows wait for the rows they depend on; otherwise one launch
                         per level.  1: always one launch per level (the cross-check of the other forms: same factor bit
                         for bit, application equal to rounding) */
} isph_schwarz_params;
void isph_schwarz_params_default(isph_schwarz_params *p);
int isph_prec_create_schwarz(isph_ctx *ctx, const isph_mat *A, const isph_schwarz_params *prm, isph_prec **M);
int isph_prec_schwarz_info(const isph_prec *M, long long info[7]);
/* which way the create call went, for tests that must know the branch a matrix reaches: [0] 1 = subdomain row lists and
 * local matrices built on the device, 0 = on the host [1] 1 = level-1 pattern built on the device, 0 = on the host (or
 * level of fill != 1) [2] 1 = the persistent sweeps split the recent words off the chunk loop (many rows beyond one chunk
 * of 96 entries on a side) [3] waves per row of the persistent factorisation, 0 = that launch did not run [4] bits of its
 * column look-up table, 0 = binary search [5] [6] runs of the persistent L / U sweep [7] [8] their throttle windows
 * [9] rows of the largest extended subdomain [10] [11] positions of the padded L / U level order */
int isph_prec_schwarz_paths(const isph_prec *M, long long out[12]);
/* wall time of the create call, ms: [0] matrix to the host [1] subdomains + local matrices [2] level-of-fill pattern
 * [3] dependency levels, orders, combine lists [4] upload [5] numeric factorisation */
int isph_prec_schwarz_timing(const isph_prec *M, double ms[6]);
int isph_prec_schwarz_export(isph_ctx *ctx, const isph_prec *M, int *rows, int *loc_ptr, long long *rowptr,
                             int *colidx, double *val);
/* Ifpack_AdditiveSchwarz<ILU(k)> with "Overlap Level" 1 across ranks (ref: precond_ifpack.h:43,60-74; Ifpack builds an
 * Ifpack_OverlappingRowMatrix from the matrix' Epetra_Import).  Aext is the square matrix of this rank's extended
 * subdomain: rows/columns [0,nlocal) = owned, [nlocal, nlocal + nghost) = the rows of the ghost columns in ghost-column
 * order, entries outside the extended column set dropped (the adapter imports those rows with the matrix' importer;
 * dist.extend_rows does it for the Python plumbing).  The halo lists are the ones of isph_mat_set_halo for the
 * un-extended matrix.  apply: gather the ghost part of r from its owners, ILU(k) solve on the extended vector (one
 * subdomain, level-scheduled path), and with combine 0 = "Add" (the wrapper's default, precond_ifpack.h:37) send the
 * ghost part of the result back to the owners, who add it; 1 = "Zero" keeps the owned part (restricted Schwarz). */
int isph_prec_create_overlap(isph_ctx *ctx, const isph_mat *Aext, int nlocal, int level_of_fill, int combine, int npeers,
                             const int *peer_rank, const int *send_ptr, const int *send_idx, const int *recv_ptr,
                             isph_prec **M);

/* Ifpack's "Precond Type" = "Chebyshev" (Ifpack_Chebyshev::ApplyInverse; ML_Cheby is the same recurrence): z = p(D^-1 A)
 * D^-1 r with the Chebyshev polynomial of degree `degree` (1..16) for the interval [alpha, beta],
 *   lambda = lambda_max (<= 0: rho = max_i sum_j |a_ij| / |a_ii|, an upper bound of the spectrum of D^-1 A; with a halo
 *   plan the all-reduced maximum over the ranks), beta = 1.1 lambda, alpha = lambda_min (<= 0: lambda / ratio),
 *   theta = (beta + alpha) / 2, delta = (beta - alpha) / 2, sigma = theta / delta, rho_0 = 1 / sigma,
 *   step 1:        w = (1 / theta) D^-1 r,  z = w                               (zero start: no matrix product)
 *   step k = 2..d: rho_k = 1 / (2 sigma - rho_{k-1}),  w = rho_k rho_{k-1} w + (2 rho_k / delta) D^-1 (r - A z),  z += w.
 * The start is always zero.  Each step k >= 2 is one sweep of the matrix with the update in the kernel's epilogue
 * (ISPH_CHEB_UNFUSED=1 at create time: a product and a vector kernel instead, for cross-checks).  A fixed linear operator:
 * any Krylov solver of isph_solve / isph_solve_block may use it.  Works on several ranks through A's halo plan (the create
 * call is then collective).  A must outlive the preconditioner: it is applied, not copied.  Fails for a matrix with a zero
 * diagonal entry.  isph_prec_create(type = "chebyshev<d>") is degree d with the other defaults (Ifpack's: degree 1,
 * ratio 30).  The recurrence is restated from the two packages' algorithm and unpinned against them.
 * value_bits (not a reference parameter): 64 (the default; 0 means the same) or 32.  With 32 the preconditioner is exactly
 * the fp64 recurrence above applied to A~ = fl32(A) in place of A: the create call rounds every stored value of A to the
 * nearest float (ties to even, subnormals kept) into a plane the preconditioner owns (4 B per stored entry), and D^-1,
 * rho, the interval and the 2d scalars all come from A~.  The sweeps stream 4 B instead of 8 B of value per entry and
 * widen each value before its fma; vectors, accumulators and the update stay double.  A~ is a fixed linear operator,
 * symmetric when A is, so every Krylov solver may still use it; the outer iteration works on the true A.  The create
 * call fails when a value exceeds the range of single precision, and with "zero diagonal" when a diagonal entry rounds
 * to 0.  A must still outlive the preconditioner (columns and slice offsets are A's).  Any other value is refused.
 * Measured at 100^3 (profiles/chebyshev_f32_100cubed.txt): one step 147.8 against 207.1 us, "chebyshev3"
 * 13.8 against 16.4 ms per solve with 22 iterations either way; not measured on more than one rank.
 * eig_type (ML's "eigen-analysis: type"): 0 (the default, "Anorm") is the rule above; 1 (ML's "cg") takes, where
 * lambda_max <= 0, lambda = min(lambda_est, rho) with lambda_est the largest real part of the Ritz values after eig_iters
 * (ML's "eigen-analysis: iterations", default 10, 1..50; at most the global row count) Arnoldi steps on D^-1 A of the
 * operator the sweeps apply -- across the halo on several ranks, the float plane with value_bits = 32.  An explicit
 * lambda_max > 0 still wins, and the 1.1 boost stays.  Departures from ML, declared: Arnoldi (classical
 * Gram-Schmidt twice per step) instead of ML's CG/Lanczos, which is meaningless for the nonsymmetric matrices of particle
 * shifting and wall rows and the same projection for a symmetric one; a deterministic start vector (first word of
 * Philox4x32-10, key (0x15B4, 0), counter (global row in the caller's numbering, level, 0, 0), u = (w + 0.5) / 2^31 - 1)
 * instead of ML's random one, so that the estimate depends neither on the library's row numbering nor on the rank count
 * up to summation rounding; and clipping by the rigorous bound rho (rho also stands when lambda_est is not finite or
 * <= 0).  The estimate stops early at an invariant subspace (h_{j+1,j} <= 1e-14 |h_00|).  Its product is one sweep with
 * the scaling in the epilogue; ISPH_EIG_UNFUSED=1 at create time runs a product and a scaling kernel instead (cross-
 * checks).  Measured at 100^3 (profiles/eig_estimate_100cubed.txt): lambda = 1.1128 where rho = 2.0000, the
 * estimate takes 2.7 ms of the create call, "chebyshev3" 17 against 22 iterations and 15.0 against 15.7 ms for create plus
 * solve; on small systems the iteration count of the stand-alone polynomial moves both ways; not timed on more than one
 * rank.  Any other eig_type or eig_iters is refused.  The string form "chebyshev<d>" keeps eig_type 0.
 * Call isph_cheb_params_default FIRST and then change fields: the struct grows at its tail. */
typedef struct {
  int degree;
  double ratio, lambda_max, lambda_min;
  int value_bits;
  int eig_type;  /* 0 = lambda from rho (default), 1 = from the Arnoldi estimate */
  int eig_iters; /* eig_type 1: Arnoldi steps, 1..50 (default 10) */
} isph_cheb_params;
void isph_cheb_params_default(isph_cheb_params *p);
int isph_prec_create_chebyshev(isph_ctx *ctx, const isph_mat *A, const isph_cheb_params *prm, isph_prec **M);
/* 32 or 64: the width of the matrix values the Chebyshev sweeps of M read (a Chebyshev preconditioner, or an AMG with
 * smoother = 2); 32 for a block ILU whose solves stream single-precision factor values ("bjacobi-ilu<k>-f32",
 * isph_ilu_params::value_bits = 32); 0 for every other preconditioner -- a plain "bjacobi-ilu<k>" included -- and for NULL. */
int isph_prec_value_bits(const isph_prec *M);
/* 32 for an AMG built with isph_amg_params::cycle_bits = 32 (its whole V cycle runs in single-precision storage; its
 * isph_prec_value_bits is 32 too); 64 for every other preconditioner and for NULL. */
int isph_prec_cycle_bits(const isph_prec *M);
/* out = {lambda_used, rho, Arnoldi steps taken} of a Chebyshev preconditioner (level 0) or of level `level` of an AMG
 * (the estimate of the level's fp64 operator: the one that damps the prolongator; with cheb_value_bits = 32 the
 * smoother's own estimate on fl32(A_l) is not reported).  With eig_type 0 -- or an explicit lambda_max -- it returns
 * {rho, rho, 0}.  Collective for a hierarchy across ranks.  Any other preconditioner, or a level out of range, is an
 * error. */
int isph_prec_eig_estimate(isph_ctx *ctx, const isph_prec *M, int level, double out[3]);

/* Belos' GMRES polynomial (GmresPolySolMgr's polynomial, restated from the algorithm and unpinned against Belos,
 * DESIGN.md 10) in D^-1 A as a fixed linear preconditioner: z = p(B) D^-1 r, B = D^-1 A, p the degree - 1 polynomial with
 * 1 - B p(B) = prod_k (1 - B / theta_k) whose roots theta_1 .. theta_degree are the harmonic Ritz values of `degree`
 * Arnoldi steps from v_0 = u / |u|.  No interval and no ratio, and a complex spectrum is handled.
 *   u: the deterministic start vector of the eigenvalue estimate (isph_cheb_params above: Philox, keyed by the global row
 *      in the caller's numbering), so the polynomial depends neither on the library's row numbering nor on the rank count
 *      up to summation rounding.  nullvec != NULL (a singular system; any length, normalised inside): u and every set-up
 *      product w are projected, w <- w - (w.n) n.
 *   Arnoldi: classical Gram-Schmidt twice per step with the solvers' deterministic multi-dot, H of size (degree + 1) x
 *      degree; H^ = H_d + h_{d+1,d}^2 f e_d^T with H_d^T f = e_d; the roots are the eigenvalues of H^ (host, the complex
 *      Hessenberg-QR the Recycling GMRES uses).  A breakdown h_{j+1,j} <= 1e-14 |h_00| at step j < degree gives degree j.
 *   Order: modified Leja -- the root of largest modulus first, then always the one farthest (by the product of distances)
 *      from those chosen, a conjugate directly behind its partner.  |Im theta| <= 1e-8 |theta| counts as a real root.
 *   Application, product form: r <- D^-1 r, z = 0; a real root: z += r / theta, r <- r - (B r) / theta; a pair a +- ib:
 *      t = 2a r - B r, z += t / (a^2 + b^2), r <- r - (B t) / (a^2 + b^2); the product behind the last root is not made:
 *      degree - 1 sweeps of the matrix, each one kernel with the update in its epilogue (ISPH_POLY_UNFUSED=1 at create
 *      time: a product and a vector kernel instead, same bits; the cross-check).  No projection in the application:
 *      B 1 = 0 keeps a null component bounded and the solver removes it.
 * degree: 1..25 (Belos' maximum); anything else is refused.  A root with |theta| <= 1e-10 max |theta| fails the create
 * call with "near-zero root: a singular matrix needs the null vector", a zero diagonal entry fails it too.  A fixed linear
 * operator: every solver type may use it.  Collective on several ranks.  A must outlive the preconditioner: it is applied,
 * not copied.  Several vectors (isph_prec_apply_multi, isph_solve with nvec > 1) are applied one after the other.
 * isph_prec_refactor takes a polynomial created under isph_ctx_hold_pattern: the whole set-up again with the null vector
 * of the create call, bit for bit a fresh create.  isph_prec_create(type = "gmres-poly<d>") is degree d without a null
 * vector.  Measured at 100^3: DESIGN.md 9.4.
 * Call isph_poly_params_default FIRST and then change fields: the struct grows at its tail. */
typedef struct {
  int degree; /* 1..25, default 4 */
} isph_poly_params;
void isph_poly_params_default(isph_poly_params *p);
int isph_prec_create_gmres_poly(isph_ctx *ctx, const isph_mat *A, const isph_poly_params *prm,
                                const double *nullvec /*[nrow] caller's numbering, h|d, or NULL*/, int on_device, isph_prec **M);
/* The polynomial of M: roots_re_im[2 k], roots_re_im[2 k + 1] = the real and the imaginary part of root k in application
 * order (room for 2 x 25), hess = H column-major with leading dimension 26 (room for 26 x 25; rows 0 .. degree of columns
 * 0 .. degree - 1 are set, the rest is 0), *degree = the degree reached.  Any argument but M may be NULL.  Another kind of
 * preconditioner is an error. */
int isph_prec_poly_info(const isph_prec *M, double *roots_re_im, double *hess, int *degree);
/* The kind a type string of isph_prec_create names (0 "none", 1 "jacobi", 2 "bjacobi-ilu<k>", 3 "sa-amg", 4 "ilu<k>",
 * 6 "chebyshev<d>", 7 "gmres-poly<d>"), or -1 for a string it refuses.  Host only: no context, no device. */
int isph_prec_type_kind(const char *type);

/* z = M^-1 r (Belos::EpetraPrecOp::Apply -> Ifpack ApplyInverse). */
int isph_prec_apply(isph_ctx *ctx, const isph_prec *M, const double *r /*[h|d]*/,
                    double *z /*[h|d]*/, int on_device);
/* z_k = M^-1 r_k for nvec vectors: r and z are column-major [lda x nvec] like the multivectors of isph_solve, nvec >= 1
 * and lda >= n (anything else is an error); rows n .. lda of z are not written.  Any preconditioner type.  Host operands
 * cross the link in one strided copy each way.
 * Where the type has a one-sweep form the vectors share the sweeps of M, with the bits of nvec calls of isph_prec_apply:
 *   - block ILU(k): 2..4 vectors in one sweep of the factor stream;
 *   - the Chebyshev polynomial (isph_prec_create_chebyshev, either value_bits) and the SA-AMG with smoother = 2 and
 *     cycle_bits = 64 (either cheb_value_bits): every step of the polynomial, every A_l, R_l, P_l, A_l P_l and the dense
 *     coarse inverse is read once per group of up to 4 vectors; the matrix values and columns are loaded once per entry,
 *     every vector does its own gather and runs the single kernels' operations in their order.
 * Applied one vector after the other: every other type, the Gauss-Seidel smoothers, cycle_bits = 32, a matrix with a halo
 * plan or ghost columns, a hierarchy across ranks, ISPH_CHEB_UNFUSED=1, nvec = 1, and any preconditioner created under
 * ISPH_PREC_MULTI_SINGLE=1 (the cross-check and the timing baseline of the one-sweep forms).  isph_solve with nvec > 1
 * and isph_solve_block apply their preconditioner by the same rule.  The K-fold work vectors come from the pool at the
 * first application to several vectors and go back with the preconditioner. */
int isph_prec_apply_multi(isph_ctx *ctx, const isph_prec *M, int nvec, const double *r /*[h|d] lda x nvec*/,
                          double *z /*[h|d] lda x nvec*/, int lda, int on_device);
/* 1 when nvec vectors share the sweeps of M in isph_prec_apply_multi / isph_solve / isph_solve_block, 0 when they are
 * applied one after the other (read-only, in the spirit of isph_prec_amg_path). */
int isph_prec_multi_path(isph_ctx *ctx, const isph_prec *M, int nvec);
/* Export the factor as CSR (strict L, D, strict U in one pattern == A's
 * in-block pattern, columns sorted) for parity tests. */
int isph_prec_export_ilu(isph_ctx *ctx, const isph_prec *M, int *rowptr, int *colidx, double *val);
long long isph_prec_nnz(const isph_prec *M);
/* sizes: [0]=factor entries [1]=triangular-solve stream chunks in use (64 entries each)
 *        [2]=stream capacity in chunks [3]=number of blocks */
int isph_prec_info(isph_ctx *ctx, const isph_prec *M, long long info[4]);
void isph_prec_destroy(isph_prec *M);

/* ---- solve ------------------------------------------------------------ */

/* Same keys and defaults as SolverLin_Belos::setParameters
 * (ref: solver_lin_belos.h:224-264).
 * basis_bits (not a reference parameter): 64 (the default; 0 means the same) or 32; any other value is refused.  With 32
 * and solver_type 0 -- flexible or not, DGKS or ICGS, one right-hand side or the lockstep solve of several -- the Krylov
 * basis is stored in single precision (the compressed-basis GMRES of the literature): v_0 = fl32(r / beta) and
 * v_{j+1} = fl32(w / |w|), round to nearest even, subnormals kept.  Every read widens the entry to double; the dots,
 * updates, norms, the DGKS decision, the Hessenberg matrix and the Givens rotations are the fp64 ones, two-stage and
 * deterministic as before.  The preconditioner and the operator get the widened ROUNDED vector (the sweep that writes
 * a float column writes it to one fp64 buffer as well), so A Z_j = V_{j+1} H_j holds for the stored vectors up to that
 * one rounding per column.  Z stays fp64 and x += Z y is unchanged; the non-flexible form is x += M^-1 (V y) with the
 * float columns widened; w, x and b stay fp64.  The null vector of a singular system stays an fp64 vector: the solve
 * takes the explicit projection y - (y.n) n after every product (what IMGS does at 64 bits) instead of carrying n as a
 * column of the basis -- chosen because it keeps every Gram-Schmidt kernel on one storage type; the deflated form was
 * not built, so the two were not timed against each other.  The basis takes 4 ld (m + 1) + 8 ld bytes instead of
 * 8 ld (m + 2), ld = the rows rounded up to 64.
 * Within one restart cycle the TRUE residual of such a solve stalls at 3-4e-8 |r0| although the recurrence residual
 * goes on falling: the rounding of v_0 and of the first columns, whose coefficients y_j are the largest.  So when the
 * recurrence residual reaches tol, the true residual |b - Op(x)| / scale is computed (the operator application a
 * restart makes, same scale as the recurrence test): <= tol is convergence, otherwise the method restarts from that
 * residual, which counts in isph_solve_info::restarts and in residual_restarts.  On the host restatement
 * (tests/krylov_cb_reference.py) one such restart costs 0-4 iterations at tol 1e-8.  max_restarts and max_iters end
 * the solve as before; with tol = 0 the confirmation never fails a converged solve.
 * Measured at 100^3 (profiles/basis_f32_100cubed.txt; FGMRES(50), DGKS, tol 1e-8, 32 against 64 bits in one
 * run): k_multi_dot 21.8 against 35.9 us and k_multi_axpy_norm 24.5 against 36.0 us per launch (0.61 and 0.68 of the time
 * for 0.52 and 0.57 of the bytes); the fused update k_multi_axpy_dot is not faster at 32 bits, 38.5 against 39.5 us.  The
 * solve: 33.89 against 34.28 ms with "bjacobi-ilu0" (72 against 71 iterations, one restart either way), but 15.62 against
 * 14.97 ms with "jacobi" (45 against 43 iterations) and 18.33 against 16.53 ms with "chebyshev3" (23 against 22), where
 * the confirmation costs one restart; pool peak 868 against 1072 MB.  Not timed on more than one rank.
 * Refused with basis_bits = 32: solver_type 1 and 2, ortho = 2 (IMGS), isph_solve_block.  With 64 or 0 the launches, the
 * arguments and the bits of x are those of a library without the field.
 * Call isph_solver_params_default FIRST and then change fields: the struct grows at its tail. */
typedef struct {
  int solver_type;   /* 0 "Block GMRES" (default), 1 "Block CG", 2 "Recycling GMRES" = GCRO-DR(num_blocks,
                        num_recycled) (solver_lin_belos.h:173-181)           */
  int flexible;      /* "Flexible Gmres" (default 1)                        */
  int num_blocks;    /* "Num Blocks" (50)                                   */
  int max_iters;     /* "Maximum Iterations" (500)                          */
  int max_restarts;  /* "Maximum Restarts" (15)                             */
  double tol;        /* "Convergence Tolerance" (1e-8)                      */
  int ortho;         /* "Orthogonalization": 0 DGKS (default), 1 ICGS, 2 IMGS */
  int verbose;       /* rank-0 status lines like Belos "Verbosity"          */
  int num_recycled;  /* "Num Recycled Blocks" (50, solver_lin_belos.h:240); solver_type 2 needs
                        0 < num_recycled < num_blocks, as Belos::GCRODRSolMgr does */
  int basis_bits;    /* storage of the Krylov basis: 64 (default; 0 means the same) or 32, see above */
} isph_solver_params;
void isph_solver_params_default(isph_solver_params *p);

typedef struct {
  int converged, iters, restarts;
  double rel_res_implicit;  /* recurrence residual / ||r0||                 */
  double rel_res_explicit;  /* ||b - A x|| / ||b|| (solver_lin_belos.h:201-212) */
  double prec_setup_ms;     /* filled by callers that build M around the solve */
  double solve_ms;          /* HIP-event time of the whole call on the stream */
  double spmv_ms;           /* sum of SpMV kernel times (profile mode only) */
  int spmv_calls;
  int reorth;               /* Gram-Schmidt steps whose second pass was applied (DGKS: when the norm dropped below
                               1/sqrt(2) of its value before the first pass; ICGS: every step), summed over the
                               right-hand sides.  IMGS always sweeps twice and is not counted: 0, as for CG */
  int residual_restarts;    /* basis_bits = 32: restarts (counted in `restarts` too) taken because the true residual was
                               still above tol when the recurrence residual had reached it; 0 with basis_bits 64 */
} isph_solve_info;

/* Replaces SolverLin_Belos::solveProblem (ref: solver_lin_belos.h:130-222):
 * singular => n = mask/||mask||, b -= (b.n)n, operator y = Ax - (Ax.n)n,
 * x -= (x.n)n; right preconditioning; non-convergence is reported in `info`,
 * never an error.  b and x are column-major [lda x nvec] exactly as
 * createLoadMultiVector / createSolutionMultiVector receive them
 * (ref: solver_lin.cpp:45-58); columns are solved one after another
 * (Belos block size 1).  x holds the initial guess on entry.
 * b is overwritten by its projection when singular, as in the reference. */
int isph_solve(isph_ctx *ctx, const isph_mat *A, const isph_prec *M,
               double *b /*[h|d]*/, double *x /*[h|d]*/, int nvec, int lda,
               int is_singular, const int *null_mask /*[h] or NULL*/,
               const isph_solver_params *prm, isph_solve_info *info, int on_device);

/* ---- Recycling GMRES: a recycle space carried from one solve to the next --------------------------------------------
 * Not a reference feature: the reference builds a new Belos::GCRODRSolMgr for every solve, so its recycling stops at
 * the end of a solve.  A handle keeps the space U a solve ends with (k or k + 1 vectors of the preconditioned variable,
 * in the CALLER's row numbering, on the device) and the next isph_solve_recycle call with that handle starts from it:
 * for a sequence of slowly changing systems (one Poisson system per time step) or for the right-hand sides of one
 * system.  The next solve spends kk operator applications on C = A M^-1 U, orthonormalises by Cholesky-QR done twice,
 * projects the initial residual and continues with cycles of m - kk steps; the convergence test stays relative to the
 * residual before the projection.  The space is dropped, the solve then being the one without a handle, when the number
 * of rows changed (reason 1), when the orthonormalisation guard trips (2: a Cholesky pivot that is not positive and
 * finite, or kk max|C^T C - I| > 1/2 before the second pass), or when it holds more vectors than the new k + 1 (3).
 * After every solve with a handle the recycle step runs once more and its space is kept, converged or not; a solve
 * whose only cycle took no more than k steps keeps nothing.  With nvec > 1 the columns after the first start from U and
 * C as the column before left them (same operator: no applications, no orthonormalisation).  One handle per sequence:
 * alternating systems (Poisson / Helmholtz) take a handle each.  On several ranks every rank passes its own handle and
 * all ranks keep or drop their spaces together.  Off unless asked for: what it gains depends on the preconditioner
 * (README, "Recycling across solves").
 *
 * isph_solve_recycle with R == NULL is isph_solve.  With a handle it takes solver_type 2 only; basis_bits = 32 and a
 * cycle_bits = 32 preconditioner are refused as in isph_solve.  isph_solve_block and isph_solve_poisson_boltzmann take
 * no handle.  The handle's dense contractions run as two kernels that sweep a block of vectors once (k_tall_gemm,
 * k_block_gram); ISPH_GCRODR_UNFUSED=1 in the environment when the handle is created keeps one launch per column
 * there (the cross-check and the timing baseline).
 *
 * isph_recycle_info: out[0] rows the space belongs to, [1] vectors held, [2] solves that started from a carried space,
 * [3] solves that dropped one, [4] reason of the last drop (0 none), [5] operator applications spent on rebuilding C in
 * the last call, [6] Arnoldi steps of the last call, [7] bytes held.  isph_recycle_reset forgets the space and the last
 * call's figures and keeps the object and its two counters.  isph_recycle_export: U, column-major [n x kk], caller's
 * numbering, to host memory. */
typedef struct isph_recycle isph_recycle;
int isph_recycle_create(isph_ctx *ctx, isph_recycle **R);
void isph_recycle_destroy(isph_recycle *R);
int isph_recycle_reset(isph_recycle *R);
int isph_recycle_info(isph_ctx *ctx, const isph_recycle *R, long long out[8]);
int isph_recycle_export(isph_ctx *ctx, const isph_recycle *R, double *U /*[h] n x kk*/);
/* Diagnostic: the reverse of isph_recycle_export -- the handle then holds these kk vectors of n rows as if a solve had left
 * them (tests hand a rank-deficient space to the guard this way).  On several ranks every rank imports the same kk. */
int isph_recycle_import(isph_ctx *ctx, isph_recycle *R, int n, int kk, const double *U /*[h] n x kk*/);
int isph_solve_recycle(isph_ctx *ctx, const isph_mat *A, const isph_prec *M,
                       double *b /*[h|d]*/, double *x /*[h|d]*/, int nvec, int lda,
                       int is_singular, const int *null_mask /*[h] or NULL*/,
                       const isph_solver_params *prm, isph_solve_info *info, int on_device, isph_recycle *R);
/* Diagnostics: the two kernels alone.  Blocks are vector-major (vector v at base + v * ld), at most 64 vectors in
 * [A | B] and at most 64 outputs; coef and G are row-major in host memory; the vectors are device memory when on_device.
 * isph_dense_tall_gemm: out[:, c] = sum_i coef[i][c] Basis_i (mode 0), out[:, c] += ... (mode 1), or A <- A coef in
 * place with coef upper triangular, pb = 0, q = pa (mode 2; out is not used).  Per output one fma chain over ascending
 * i, from 0.0 or from the stored value.  Mode 3 is mode 0 by one launch per block and column, the launches a solve
 * without a handle makes: the same bits, the timing baseline.  isph_dense_block_gram: G[a][c] = sum over this rank's
 * rows of X_a Y_c, X = [XA | XB]; the same bits on every call.  per_column: by one multi-dot launch per block and column
 * of Y (at most 63 vectors per block, one rank): the timing baseline; its sums run in another order. */
int isph_dense_tall_gemm(isph_ctx *ctx, int n, int pa, double *A /*[h|d]*/, long long lda, int pb, const double *B /*[h|d]*/,
                         long long ldb, int q, const double *coef /*[h]*/, double *out /*[h|d]*/, long long ldo, int mode,
                         int on_device);
int isph_dense_block_gram(isph_ctx *ctx, int n, int pa, const double *XA /*[h|d]*/, long long lda, int pb,
                          const double *XB /*[h|d]*/, long long ldb, int q, const double *Y /*[h|d]*/, long long ldy,
                          double *G /*[h]*/, int per_column, int on_device);
/* profile mode: HIP events on the library's stream around the launches of the hot kernels, by class:
 *   [0] SpMV (k_sell_spmv16 incl. the halo exchange when there is one)   [1] preconditioner application (block ILU:
 *   k_ilu_solve_stream)   [2] k_multi_dot   [3] k_multi_axpy_dot   [4] k_multi_axpy_norm (the three sweeps of one
 *   DGKS step)   [5] k_ilu_extract   [6] k_ilu_schedule   [7] k_ilu_factor (set-up of the block ILU).
 * isph_ctx_set_profile switches the mode and starts a new collection; isph_ctx_profile_read synchronises the stream,
 * returns milliseconds and launch counts per class since the collection started, and starts the next one.
 * isph_solve_info::spmv_ms / spmv_calls are class 0 of that one solve.  No reference counterpart (the reference's
 * Teuchos timers stop at "ISPH: solvePoisson", utils.cpp:37-38). */
int isph_ctx_set_profile(isph_ctx *ctx, int on);
/* Between isph_ctx_hold_neighbours(ctx, 1) and isph_ctx_hold_neighbours(ctx, 0) the caller guarantees that the neighbour
 * list it passes in isph_particles (the same neigh_ptr / neigh_idx arrays, on the device) does not change: the layout the
 * row kernels read -- slice-transposed, ordered by matrix column for the assemblies -- is then built by the first operator
 * call and reused by the following ones, instead of once per call.  What LAMMPS' neighbour list is to the reference's
 * functors between two re-neighbourings (pair_isph.cpp: every functor of a time step walks the same list->firstneigh).
 * Either call drops what was kept.  Without it every call is self-contained. */
int isph_ctx_hold_neighbours(isph_ctx *ctx, int on);
int isph_ctx_profile_read(isph_ctx *ctx, double ms[8], int calls[8]);
/* profile mode, products of a matrix with a halo plan (more than one rank): per product the time from "boundary values
 * packed" to "ghost values landed" on the halo stream (ms[0], summed over `calls` products), the time the interior slices
 * took on the compute stream from the same instant (ms[1]), and the part of the exchange that was not hidden behind them,
 * max(0, exchange - interior) (ms[2]).  Starts the next collection.  No reference counterpart (Epetra's Import is
 * synchronous inside Epetra_CrsMatrix::Apply, solver_lin.h:133). */
int isph_ctx_halo_profile_read(isph_ctx *ctx, double ms[3], int *calls);
/* info: [0] transport of the context: 0 none (one rank), 1 RCCL, 2 host-staged  [1] ranks -- ncclCommCount of the
 * communicator for transport 1  [2] this rank (ncclCommUserRank)  [3] device (ncclCommCuDevice) */
int isph_ctx_comm_info(const isph_ctx *ctx, long long info[4]);

/* ---- row numbering ----------------------------------------------------- */

/* The reference's matrix rows follow LAMMPS' atom order (the Epetra map is atom->tag[0..nlocal), ref:
 * pair_isph.cpp:1258-1259) and Ifpack's subdomains are the bricks of the MPI decomposition (ref: precond_ifpack.h:60-74).
 * ISPH_ORDER_BRICKS (the default): every assembly entry point (isph_assemble_poisson / _helmholtz / _block_helmholtz and
 * the scalar callers) sorts the rank's owned particles into bricks of about 500 particles by their coordinates
 * (10 x 10 x 5 mean spacings in 3-D, 22 x 22 in 2-D; x fastest inside a brick; over-full bricks split) and builds the
 * matrix in that numbering -- whatever order the caller's atoms are in.  Nothing of it is visible at this boundary: b, x
 * and the null mask of isph_solve, x / y of isph_spmv, r / z of isph_prec_apply, the null vector of isph_prec_create_amg,
 * the send list of isph_mat_set_halo and the exports isph_mat_export_csr / _rows are in the caller's numbering (ghost
 * columns are never renumbered).  The bricks are the subdomains of "bjacobi-ilu<k>" when isph_prec_create is called with
 * block_size 0.  While the neighbour list is held (isph_ctx_hold_neighbours) the order of the first assembly serves the
 * following ones.  Internals exported for tests (isph_prec_export_ilu, isph_prec_amg_*) are in the matrix' numbering;
 * isph_mat_ordering gives the permutation.
 * ISPH_ORDER_CALLER: rows stay in the caller's atom order (rounds 1-4; subdomains then are `block_size` consecutive rows
 * or the caller's table, isph_prec_create_blocks).  Matrices from isph_mat_create_csr are always in the caller's order. */
#define ISPH_ORDER_CALLER 0
#define ISPH_ORDER_BRICKS 1
int isph_ctx_set_ordering(isph_ctx *ctx, int mode);
/* Optional, for ISPH_ORDER_BRICKS: the caller's periodic box (LAMMPS: domain->boxlo / boxhi / periodicity; on more than one
 * rank set periodic[a] only for axes the rank's sub-domain spans alone).  Atoms that have just wrapped around a periodic
 * box end sit at the other end of the coordinate range -- half a lattice plane at x = L - eps, the other half at +eps --,
 * which stretches the bounding box the bricks are cut from by a spacing and leaves bricks of 9 ... 11 planes per axis
 * instead of 10 (all subdomains then pay for the largest one's LDS).  With the box the sort takes coordinates relative to a
 * point in the widest empty stretch of each periodic axis, modulo the period.  NULL arguments forget the box.  Without the
 * call everything works, with uneven bricks in that situation.  No reference counterpart. */
int isph_ctx_set_periodic_box(isph_ctx *ctx, const double lo[3], const double hi[3], const int periodic[3]);
/* what the sort was made with: cell(a) = number of faces of axis a that are <= x_a (isph_mat_ordering_faces: ncell[a] - 1
 * ascending doubles), brick(a) = cell(a) / cells_per_brick[a]; key = ((brick_z * nbrick[1] + brick_y) * nbrick[0] +
 * brick_x) * (cells per brick) + (cz' * cpb[1] + cy') * cpb[0] + cx' with c' = cell mod cells_per_brick; rows ascend by
 * key, ties in the caller's order.  The faces are quantiles of the owned particles' coordinates: face k of an axis is the
 * upper edge lo + (j + 1) / inv_bin of the first bin j of the histogram bin(x) = clamp(floor((x - lo) * inv_bin), 0,
 * nbins - 1) at which the cumulative count reaches ceil(k n / ncell). */
typedef struct {
  int dim;
  double lo[3], inv_bin[3];
  int nbins[3], ncell[3], cells_per_brick[3], nbrick[3];
  double shift[3], period[3]; /* every coordinate enters as t = x - shift, + period when t < 0 (isph_ctx_set_periodic_box; period 0: as is) */
} isph_order_geometry;
/* info: [0] 1 when A carries the library's numbering (0: the caller's) [1] rows [2] subdomains; geom may be NULL */
int isph_mat_ordering_info(const isph_mat *A, long long info[3], isph_order_geometry *geom);
/* perm[r] = the caller's row held by internal row r ([nrow], may be NULL); block_ptr [subdomains + 1] (may be NULL).
 * Fails for a matrix in the caller's numbering. */
int isph_mat_ordering(isph_ctx *ctx, const isph_mat *A, int *perm, int *block_ptr);
/* faces[0 .. ncell[axis] - 2] of one axis (host array of the caller) */
int isph_mat_ordering_faces(const isph_mat *A, int axis, double *faces);

/* ---- assembly --------------------------------------------------------- */

/* Particle view = the LAMMPS arrays the reference functors capture
 * (ref: functor.h:86-104) flattened; all pointers [h|d] per `on_device`. */
typedef struct {
  int dim, nlocal, nall, ntypes;
  int kernel;              /* 0 Wendland, 1 Quintic, 2 Cubic (kernel_*.h)     */
  const double *x;         /* [nall][3]  atom->x                              */
  const int *type;         /* [nall]     atom->type (1-based)                 */
  const int *kind;         /* [ntypes+1] getParticleKind(type)  (host always) */
  const double *h;         /* [(ntypes+1)^2] pair->h            (host always) */
  const double *cutsq;     /* [(ntypes+1)^2] pair->cutsq        (host always) */
  const int *neigh_ptr;    /* [nlocal+1] flattened list->firstneigh           */
  const int *neigh_idx;    /* neighbour indices into [0,nall)                 */
  const int *colmap;       /* [nall] matrix column of particle j              */
  const double *vfrac;     /* [nall] atom->vfrac (NULL: computed on device)   */
  const double *Gc;        /* [nlocal][dim*dim] or NULL (AntiSymmetric family): only the rows of owned particles are
                            * read (the reference's Gc[nmax] holds nothing else: computePre fills local rows and
                            * does no forward comm of them, pair_isph_corrected.cpp:302-369)                        */
  const double *Lc;        /* [nlocal][dimL]    or NULL                         */
  /* ns.boundary == MorrisHolmes (pair_isph.h:125-132): fluid-solid pairs are weighted by
   * MirrorMorrisHolmes::computeMirrorCoefficient (mirror_morris_holmes.h:39-52) -- in the
   * divergence of the Poisson RHS and in the Laplacian of the Helmholtz matrix */
  int morris_holmes;       /* 0 = MirrorNothing                               */
  const double *pnd;       /* [nall] particle number density (pair->pnd) or NULL */
  double morris_safe_coeff;/* pair->morris_safe_coeff (default 0.43301)       */
  /* wall normals (pair->normal, [nall][3]) or NULL.  With a singular-Poisson mode other than
   * NotSingular the Solid rows receive the homogeneous-Neumann operator -dt n.grad
   * (ref: functor_incomp_navier_stokes_poisson.h:98-107, functor_gradient_dot_operator_matrix.h:39-79);
   * needs Gc.  solid_normal_diag = what A.diagonal[i] holds for such a row when the Poisson functor
   * runs: the functor does not assign it (:137-147); it is 1 after the scalar Helmholtz pass of the
   * same step, 0 if only block matrices were built. */
  const double *normal;
  double solid_normal_diag;
  /* 64-bit offsets of the flattened neighbour list, used instead of neigh_ptr when non-NULL: the reference's
   * largest configuration (bcc lattice, Quintic cut 3h: 748 neighbours x 4 M particles = 3e9 list entries,
   * sph-script/pore-scale-flow-3d.lmp) does not fit 32-bit offsets.  neigh_ptr may be NULL then. */
  const long long *neigh_ptr64;
} isph_particles;

/* Replaces PairISPH_Corrected::computePoisson -> FunctorOuterIncompNavierStokesPoisson
 * (ref: pair_isph_corrected.cpp:969-1015, functor_incomp_navier_stokes_poisson.h:52-181)
 * including FunctorOuterGraph (functor_graph.h:38-99), the Laplacian rows
 * (functor_laplacian_matrix.h:73-316) and the divergence RHS
 * (functor_divergence.h:54-124).  antisym=1 is the momentum-preserving family
 * (default, pair_isph.cpp:1779).  singular_mode: 0 NotSingular, 1 NullSpace,
 * 2 PinZero, 3 DoubleDiag (pair_isph.h:134-138).  ncol = number of matrix
 * columns (owned + ghost).  b_out: nlocal entries. */
int isph_assemble_poisson(isph_ctx *ctx, const isph_particles *P, int antisym, double dt,
                          const double *rho /*[nall]*/, const double *vstar /*[nall][3]*/,
                          int singular_mode, int is_rank0, int ncol,
                          isph_mat **A_out, double *b_out /*[h|d]*/, int on_device);
/* Replaces PairISPH_Corrected::computeHelmholtz -> FunctorOuterIncompNavierStokesHelmholtz
 * (ref: pair_isph_corrected.cpp:868-925, functor_incomp_navier_stokes_helmholtz.h:52-159) for the
 * NoBoundaryCond/HomogeneousNeumann family: A = I - theta dt (1/rho) div(nu rho grad .),
 * b = v + (1-theta) dt (1/rho) div(nu rho grad v) + dt (f/rho + g) - dt/rho grad p.
 * v, force: [nall][3] (atom->v, atom->f, ghosts included); nu, rho, pres: [nall];
 * g: 3 doubles (host).  b_out: column-major [lda x dim] like the reference's
 * b multivector (pair_isph.cpp:936-946); the result feeds isph_solve(nvec=dim).
 * A_out == NULL: only b is formed (theta = 0, where the reference copies b into x, pair_isph.cpp:964-966). */
int isph_assemble_helmholtz(isph_ctx *ctx, const isph_particles *P, int antisym, double dt, double theta,
                            const double *nu, const double *rho, const double *pres, const double *force,
                            const double *g, int incremental_pressure, const double *v, int ncol,
                            isph_mat **A_out, double *b_out /*[h|d]*/, int lda, int on_device);
/* The two scalar callers of the same solver objects, built on the same Laplacian rows:
 * PairISPH_Corrected::computeSoluteTransportSpecies -> FunctorOuterSoluteTransport (ref: pair_isph_corrected.cpp:844-861,
 * functor_solute_transport.h:47-138; solved at pair_isph.cpp:811-835):  (I - theta dt D lap) c_new = c + (1-theta) dt D lap c
 * on the rows of kind Fluid, unit rows for Solid / BufferDirichlet / BufferNeumann particles (b = c there); the Laplacian
 * couples a Fluid row to Fluid and buffer neighbours, not to Solid ones (FilterMatchBinary(Fluid, Fluid - BufferNeumann):
 * the neighbour mask is only consulted for Solid neighbours, functor_laplacian_matrix.h:143-146).  conc: [nall];
 * b_out: [nlocal].  Kinds in P->kind may be 99 Fluid, 12 Solid, 32 BufferDirichlet, 64 BufferNeumann (pair_isph.h:113-124). */
int isph_assemble_solute_transport(isph_ctx *ctx, const isph_particles *P, int antisym, double dt, double theta,
                                   double dcoeff, const double *conc /*[h|d]*/, int ncol, isph_mat **A_out,
                                   double *b_out /*[h|d]*/, int on_device);
/* PairISPH_Corrected::computeAppliedElectricPotential -> FunctorOuterAppliedElectricPotential (ref:
 * pair_isph_corrected.cpp:569-620, functor_applied_electric_potential.h:36-98; solved at pair_isph.cpp:635-657):
 * -div(sigma grad phi) = 0 on the Fluid rows (FilterMatchBinary(Fluid, Fluid)), unit rows with b = phi on the buffer
 * particles (the Dirichlet data), unit rows with b = 0 on Solid ones.  sigma: [nall] conductivity or NULL (= 1);
 * phi: [nall]; b_out: [nlocal]. */
int isph_assemble_applied_potential(isph_ctx *ctx, const isph_particles *P, int antisym, const double *sigma /*[h|d]*/,
                                    const double *phi /*[h|d]*/, int ncol, isph_mat **A_out, double *b_out /*[h|d]*/,
                                    int on_device);
/* Replaces PairISPH_Corrected::computeBlockHelmholtz -> FunctorOuterIncompNavierStokesBlockHelmholtz
 * (ref: pair_isph_corrected.cpp:941-964, functor_incomp_navier_stokes_block_helmholtz.h:57-187) with the block branch
 * of the Laplacian functor (functor_laplacian_matrix.h:269-314) and FunctorOuterBoundaryNavierSlip
 * (functor_boundary_navier_slip.h:53-184): the dim x dim blocks A_blk(ib,jb) of the velocity Helmholtz system with
 * wall rows distributed by the wall normals, exactly as the reference writes them (csrc/block_helmholtz.hpp lists
 * the steps).  normal: [nall][3] wall normals (pair->normal) or NULL; beta: ns.beta (slip length factor).
 * blocks_out[ib*dim+jb] receives block (ib,jb) on the scalar pattern; without normals the off-diagonal blocks are
 * zero and returned as NULL.  b_out: column-major [lda x dim].  The result feeds isph_solve_block. */
int isph_assemble_block_helmholtz(isph_ctx *ctx, const isph_particles *P, int antisym, double dt, double theta,
                                  double beta, const double *nu, const double *rho, const double *pres,
                                  const double *force, const double *g, int incremental_pressure, const double *v,
                                  const double *normal, int ncol, isph_mat **blocks_out, double *b_out, int lda,
                                  int on_device);
/* FunctorOuterVolume (ref: functor_volume.h:40-80); vfrac_out [nlocal]. */
int isph_compute_volumes(isph_ctx *ctx, const isph_particles *P, double *vfrac_out, int on_device);
/* Particle number density of the MorrisHolmes mirror, the `pnd` member of isph_particles: W(0) + sum of W(r_ij) over the
 * neighbours that are not of the opposite phase (FunctorOuterNormal, ref: functor_normal.h:57-133, called by
 * PairISPH_Corrected::computeNormals, pair_isph_corrected.cpp:396-419); pnd_out [nlocal], ghosts by forward comm. */
int isph_compute_pnd(isph_ctx *ctx, const isph_particles *P, double *pnd_out, int on_device);

/* FunctorOuterGradientCorrection + FunctorOuterLaplacianCorrection
 * (ref: functor_gradient_correction.h:23-71, functor_laplacian_correction.h:24-153,
 * pair_isph_corrected.cpp:333-369): G_i [nlocal][dim*dim] column-major and L_i
 * [nlocal][dimL] packed upper for the owned particles; P->vfrac must hold the
 * ghosts' volumes already (forward comm). */
int isph_compute_corrections(isph_ctx *ctx, const isph_particles *P, double *Gc_out, double *Lc_out, int on_device);

/* ---- streaming operators either side of the solve -------- */

/* Corrected::FunctorOuterGradient<.,AntiSymmetric?> (ref: functor_gradient.h:78-170): f [nall] ->
 * grad_out [nlocal][3].  use_filter/filt_i/filt_j = FilterBinary particle-kind masks (filter.h:37-54). */
int isph_gradient(isph_ctx *ctx, const isph_particles *P, int antisym, const double *f, double alpha,
                  int use_filter, int filt_i, int filt_j, double *grad_out, int on_device);
/* Corrected::FunctorOuterDivergence (ref: functor_divergence.h:54-124): f [nall][3] -> div_out [nlocal]. */
int isph_divergence(isph_ctx *ctx, const isph_particles *P, int antisym, const double *f, double alpha,
                    int use_filter, int filt_i, int filt_j, double *div_out, int on_device);
/* PairISPH_Corrected::correctVelocity + correctPressure (ref: pair_isph_corrected.cpp:1020-1050,
 * functor_correct_velocity.h, functor_correct_pressure.h): vstar [nall][3] (owned rows updated),
 * p [nall] (all updated), dp [nall] with ghost values. */
int isph_correct_velocity_pressure(isph_ctx *ctx, const isph_particles *P, int antisym, double dt,
                                   const double *rho, const double *dp, double *vstar, double *p,
                                   int incremental_pressure, int on_device);
/* PairISPH_Corrected::advanceTime (ref: pair_isph_corrected.cpp:1172-1199): begin computes
 * dp_out[nlocal] = grad p . dt/2 (vnp1+v); the caller forward-communicates it; end applies
 * p += dp, x += dt/2 (vnp1+v), v = vnp1 to the first `count` atoms. */
int isph_advance_begin(isph_ctx *ctx, const isph_particles *P, int antisym, double dt, const double *p,
                       const double *v, const double *vnp1, double *dp_out, int on_device);
int isph_advance_end(isph_ctx *ctx, int count, int dim, double dt, const double *dp, const double *vnp1,
                     double *p, double *x, double *v, int on_device);

/* SolverLin_Belos::solveBlockProblem (solver_lin_belos.h:53-128) over the blocks SolverLin::setBlock collects
 * (solver_lin.cpp:127-138): blocks[i*dim+j] is block (i,j) of the dim x dim operator (NULL = zero block, diagonal
 * blocks required), b and x are column-major [lda x dim] like the reference's multivectors, M (may be NULL) is
 * applied to every component -- the block-diagonal preconditioner PrecondWrapper_ML::create(dim) builds
 * (precond_ml.h:138-155).  Singular systems are not supported, as in the reference (:60-61). */
int isph_solve_block(isph_ctx *ctx, int dim, const isph_mat *const *blocks, const isph_prec *M, double *b, double *x,
                     int lda, const isph_solver_params *prm, isph_solve_info *info, int on_device);

/* ---- smoothed-aggregation AMG in place of PrecondWrapper_ML (precond_ml.h:40-171) ----
 * Parameters mirror the keys the wrapper sets (precond_ml.h:44-55): "max levels" 5, "aggregation: type" Uncoupled,
 * "smoother: type" symmetric Gauss-Seidel with "smoother: sweeps" 1 pre and post, direct coarse solve; plus ML's
 * defaults "coarse: max size" 128, "aggregation: damping factor" 4/3, "aggregation: threshold" 0.  `block` is the
 * row-block the Gauss-Seidel sweeps are local to (ML: the processor).  nullvec != NULL restates
 * PrecondWrapper_ML::setNullVector (precond_ml.h:97-127): one pre-computed null-space vector, smoother as the
 * coarse solver.  The hierarchy is rebuilt on every create, like the reference does on every solve.
 * More than one rank (a context with a communicator, A with its halo plan set): the call is COLLECTIVE.  Aggregates and
 * prolongator stay on the rank (Uncoupled), the coarse operators are P^T A P with the whole A -- ghost columns and a halo
 * plan per level, derived from A's -- and the coarsest systems of all ranks are solved as one (a dense inverse on every
 * rank; the smoother when nullvec is given).  Every rank must call it, with the same parameters.
 * Call isph_amg_params_default FIRST and then change fields: the struct grows at its tail. */
typedef struct {
  int max_levels, coarse_max;
  double omega;
  int block, sweeps;
  double theta;
  /* "smoother: type": 0 = symmetric Gauss-Seidel, `sweeps` symmetric sweeps before and after the coarse correction
   * (the wrapper's default, precond_ml.h:50-52); 1 = "ML Gauss-Seidel" / "Gauss-Seidel" with "smoother: Gauss-Seidel
   * efficient symmetric" (the ml.xml of the reference's benchmark protocol, bench-script/hopper/tgv/1728/ml.xml):
   * `sweeps` FORWARD sweeps before the coarse correction, `sweeps` BACKWARD sweeps after it.  (With a null vector the
   * coarsest level is still solved by symmetric sweeps.)
   * 2 = "Chebyshev" ("MLS" is ML's old name for it): a Chebyshev polynomial of degree `sweeps` (ML's meaning of
   * "smoother: sweeps" for this smoother, at most 16) in D^-1 A before and after the coarse correction, on the interval
   * [rho / cheb_ratio, 1.1 rho] with rho = ||D^-1 A||_inf of the level (see isph_cheb_params for the recurrence).  No
   * Gauss-Seidel factor is built and `block` is not used; the hierarchy is the one smoother 0 builds, bit for bit.  The
   * polynomial of one level depends neither on the row order nor on the rank count (rho is all-reduced); the AMG result
   * as a whole still does, because the Uncoupled aggregates, and with them the cycle, follow the decomposition.  The
   * cycle is a fixed linear operator, symmetric for a symmetric matrix: "Block CG" may use it.  With a null vector the coarsest level is "solved" by the same polynomial.
   * Departures from ML: by default (eig_type 0) lambda_max is the Anorm bound rho, not ML's 10 CG steps; eig_type 1 gives
   * ML's rule with Arnoldi in place of CG, a deterministic start vector and clipping by rho (see eig_type below and
   * isph_cheb_params).  The 1.1 boost is kept on top either way.
   * 4 = "IFPACK" with "smoother: ifpack type" = "ILU" and "smoother: ifpack overlap" = 0 (sph-script/ml-ifpack.xml): block
   * ILU(ilu_fill) Richardson sweeps.  One step is x += (L_B U_B)^-1 (b - A_l x), from a zero guess x = (L_B U_B)^-1 b;
   * `sweeps` of them before and `sweeps` after the coarse correction, the first post-sweep on r -= (A P) e where A_l P_l
   * is kept, as with smoother 0.  L_B U_B is the block-Jacobi ILU(ilu_fill) of A_l, what "bjacobi-ilu<k>" builds, on the
   * blocks of the Gauss-Seidel smoothers: `block` rows on level 0, 64 rows on coarse levels (there as dense 64 x 64
   * inverses up to 32768 rows, through the chunk stream above that and on level 0).  The hierarchy is the one smoother 0
   * builds.  Departures from ML: ML hands Ifpack the rank's whole matrix, this factor is local to the blocks; with a null
   * vector the coarsest level is solved by `sweeps` symmetric Gauss-Seidel sweeps (the rule of smoother 1) -- the ILU of
   * a small singular coarsest block is its complete LU; a level with a row that stores no diagonal entry is smoothed by
   * smoother 0's Gauss-Seidel on that rank (isph_prec_amg_path shows it).  A pivot that becomes zero numerically is not
   * guarded on the stream levels, as in "bjacobi-ilu<k>" and in Ifpack.  Not symmetric: not for "Block CG".  ML's
   * smoother loop (zero-guess shortcut, then residual plus correction per sweep) is restated from ML's published
   * algorithm and is not pinned against Trilinos.  cycle_bits = 32 and cheb_value_bits = 32 are refused with it.  (The value 3 names no
   * smoother and is refused, as it always was.)
   * Measured at 100^3 (profiles/amg_ilu_100cubed.txt, create + solve): ILU(0), 1 sweep: 32 iterations, 15.1 + 29.9 ms
   * (smoother 0: 33 iterations, 12.4 + 30.9 ms); 3 sweeps: 19 iterations, 15.1 + 44.5 ms; ILU(1), 1 sweep: 32 iterations,
   * 59.1 + 41.5 ms.  No faster than smoother 0 there: not the default. */
  int smoother;
  double cheb_ratio; /* smoother 2: "smoother: Chebyshev alpha", lambda_max / lambda_min of the interval; default 20 */
  /* smoother 2 only (not read otherwise): 64 (default; 0 means the same) or 32 = the polynomial of every level (the
   * coarsest included when a null vector is given) is that of fl32(A_l), see isph_cheb_params::value_bits.  Only the
   * smoother's sweeps read floats: aggregates, P, the Galerkin products, residuals, restriction, prolongation and the
   * dense coarse inverse stay fp64, and the hierarchy is bit for bit the one cheb_value_bits = 64 builds.  The
   * post-smoother then forms b - fl32(A) x in a sweep of its own (the A P shortcut holds the residual of A); on one rank
   * that takes back what the floats save: 29.4 against 29.9 ms per solve at 100^3, 26 iterations either way. */
  int cheb_value_bits;
  /* "eigen-analysis: type" / "eigen-analysis: iterations".  eig_type 0 (default, "Anorm"): rho as above.  1 (ML's "cg"):
   * EVERY level l uses lambda_l = min(lambda_est, rho) of its own operator (isph_cheb_params::eig_type; the start vector's
   * counter carries the level, and on coarse levels the level's own row index plus the rank offset) for the prolongator
   * damping omega / lambda_l, whatever the smoother, and for the Chebyshev interval [lambda_l / cheb_ratio, 1.1 lambda_l]
   * of smoother 2.  With cheb_value_bits = 32 the damping uses the estimate of A_l (the hierarchy stays fp64) and the
   * smoother the estimate of fl32(A_l).  eig_iters: 1..50, default 10.  isph_prec_eig_estimate reads the numbers back.
   * "sa-amg" keeps eig_type 0.  Measured at 100^3 (profiles/eig_estimate_100cubed.txt; lambda 1.11 / 1.28 / 1.32 where rho is
   * 2.00 / 2.23 / 2.10): smoother 2 of degree 2 needs 17 against 26 iterations, 33.1 against 38.4 ms for create plus solve
   * (create 14.6 against 10.3 ms); smoother 0 needs 27 against 33 iterations, 41.6 against 43.1 ms. */
  int eig_type, eig_iters;
  /* 64 (default; 0 means the same) or 32 = the whole V cycle in single-precision STORAGE: operators, level vectors and
   * gathers are float, all arithmetic stays fp64.  With 64 or 0 the launches, arguments and bits of every result are those
   * of a library without the field.  Needs smoother = 2; any other width, or 32 with another smoother (the Gauss-Seidel
   * stream and the dense block smoothers keep fp64 vectors), is refused by the create call.  Off by default.
   * The arithmetic with cycle_bits = 32, smoother = 2:
   *   Hierarchy.  Aggregates, P, R, the Galerkin products, the eigenvalue estimates of A_l, the damping and the exported
   *     levels are the fp64 ones, bit for bit those of cycle_bits = 64.
   *   Float planes.  After the set-up every operator the cycle applies gets a float plane, each stored value rounded once
   *     (nearest even, subnormals kept, element positions unchanged): A~_l = fl32(A_l), the plane cheb_value_bits = 32
   *     makes; P~_l = fl32(P_l); R~_l = P~_l^T; and on the levels that keep A P (one rank, no halo), fl32(A_l P_l) of the
   *     set-up's product.  A value beyond FLT_MAX fails the create call; a diagonal that rounds to 0 fails as a zero
   *     diagonal, as cheb_value_bits = 32 does.
   *   Scalars and diagonal.  D^-1 of a level is stored as float, fl32(1 / a~_ii) with the quotient taken in fp64.  rho, the
   *     interval and the Chebyshev scalars come from A~_l exactly as cheb_value_bits = 32 takes them, the second Arnoldi
   *     estimate on fl32(A_l) with eig_type = 1 included; cheb_value_bits itself is not read.
   *   Stored vectors.  Every level vector is float: x, b, r of the cycle and w, y of the polynomial.  Every kernel widens its
   *     operands to fp64, does all arithmetic in fp64 and rounds ONCE per stored element.  A product of two floats is exact
   *     in fp64, so a row sum is an fp64 sum of exact products.  In a Chebyshev step wn is computed in fp64; then
   *     w = fl32(wn) and yout = fl32(y + wn) with the unrounded wn.
   *   Entry, exit, coarsest solve.  b_0 = fl32(r) of the Krylov vector; z = the float result widened.  The coarsest dense
   *     inverse stays fp64; it reads the float b and writes fl32(x).  Across ranks the right-hand side is widened and the
   *     all-reduce stays fp64.  With a null vector the coarsest level runs the same float polynomial.
   *   Cycle order, unchanged: (1) pre-smoother from a zero guess (product-free first step); (2) r = fl32(b - A~ x);
   *     (3) b_c = fl32(R~ r); (4) recursion; (5) x = fl32(x + P~ e); (6) where A P is kept, r = fl32(r - fl32(A P) e) feeds
   *     the post-smoother's first step, otherwise that step forms b - A~ x itself.
   *   Halo.  Ghost values travel as doubles, widened in the pack kernel: a ghost read in a sweep is a double that holds a
   *     float.
   * The cycle is NOT a linear operator (it rounds): isph_solve and isph_solve_block take such a preconditioner only with
   * flexible GMRES (solver_type 0, flexible 1: the default); solver_type 1 or 2, or flexible = 0, is refused there with
   * cycle_bits named -- x += M^-1 (V y) would apply the rounded cycle to a vector it was never applied to.
   * isph_solve_poisson_boltzmann passes the pair through and keeps the same rule. */
  int cycle_bits;
  /* smoother 4 only (not read otherwise): "fact: level-of-fill" of the sublist "smoother: ifpack list", 0..8; default 0,
   * Ifpack's.  Any other value is refused by the create call. */
  int ilu_fill;
} isph_amg_params;
void isph_amg_params_default(isph_amg_params *p);
int isph_prec_create_amg(isph_ctx *ctx, const isph_mat *A, const isph_amg_params *prm, const double *nullvec,
                         int on_device, isph_prec **M);
/* test/diagnostic access: info = {rows, nnz(A_l), nnz(P_l)}; what: 0 = A_l, 1 = P_l (CSR, columns ascending) */
int isph_prec_amg_levels(const isph_prec *M);
int isph_prec_amg_info(isph_ctx *ctx, const isph_prec *M, int level, long long info[3]);
int isph_prec_amg_export(isph_ctx *ctx, const isph_prec *M, int level, int what, int *rowptr, int *colidx, double *val);
int isph_prec_amg_aggregates(isph_ctx *ctx, const isph_prec *M, int level, int *agg);
/* which branch of every ladder the set-up took on `level` (read-only; host integers the set-up counted as it went):
 *   out[0] MIS rounds of the aggregation, out[1] how many of them ran on work lists (0 / 0 on the coarsest level);
 *   out[2] prolongator: 16 or 64 = one pass with that many lanes per row, 2 = the two passes;
 *   out[3] the kernel that gave A P: 1 rows<64>, 2 rows<256>, 3 table<256>, 4 table<1024>, 5 table<4096>;
 *   out[4] Galerkin product R (A P): 1 direct-addressed table, 2 hashed (more than 4096 coarse columns);
 *   out[5] smoother: 0 none (coarsest level, direct solve), 1 dense 64-row blocks, 2 chunk stream, 3 Chebyshev,
 *          4 block ILU(k) as dense 64-row block inverses, 5 block ILU(k) through the chunk stream (smoother 4; a level
 *          it smoothes by Gauss-Seidel -- a coarsest level it has to solve, a row without a diagonal -- reports 1 or 2);
 *   out[6] coarsest level only: 1 dense direct solve, 2 the smoother;
 *   out[7] preparation of the aggregation: 1 inside the SELL -> CSR sweep, 2 one sweep over the CSR copy (threshold 0),
 *          3 separate kernels (threshold > 0).
 * Entries 0, 1, 2, 3, 4 and 7 are 0 on the coarsest level (and on a level whose coarsening was given up).  With several
 * ranks, a level that a rank passes on unchanged (it cannot coarsen while others can: P = I) keeps out[2] = 0 on that
 * rank while out[3] and out[4] name the kernels of its products; out[0], out[1] and out[7] describe the aggregation it
 * tried. */
int isph_prec_amg_path(isph_ctx *ctx, const isph_prec *M, int level, long long out[8]);
/* isph_prec_refactor calls this hierarchy has gone through (0 for any other preconditioner) */
long long isph_prec_amg_refreshes(const isph_prec *M);
/* New values for the null vector of a hierarchy that was created with one (n doubles, the caller's row numbering), read by
 * the next isph_prec_refactor: PrecondWrapper_ML::setNullVector before a ReComputePreconditioner.  The cycle is not
 * touched by this call alone.  REFUSED for a hierarchy created without a null vector. */
int isph_prec_amg_set_nullvec(isph_ctx *ctx, isph_prec *M, const double *nullvec /*[h|d]*/, int on_device);

/* ---- nonlinear Poisson-Boltzmann: PairISPH::computePoissonBoltzmann (ref: pair_isph.cpp:573-600, every step when
 * enabled, :1312-1313) and the NOX solve it drives through SolverNOX_Stratimikos (pair_isph.h:78).
 *   F_i = (-div(eps grad psi))_i + kappa^2 g(psi_i) + f_i  on the rows of kind Fluid, BufferDirichlet, BufferNeumann
 *         (exact kind match, functor_poisson_boltzmann_f.h:40-86, pair_isph_corrected.cpp:439-484); the Laplacian is the
 *         corrected (antisym = 0) or AntiSymmetric family with FilterBinary(Fluid, All), the MorrisHolmes mirror when
 *         P->morris_holmes is set (FunctorPoissonBoltzmannF_MorrisHolmes);
 *   F_i = psi0_i - psi_i                                  on the rows of kind Solid and Boundary;
 *   g(psi) = sinh(psi) / (1 + 2 gamma sinh^2(psi/2)), linearized: psi / (1 + 2 gamma (psi/2)^2);
 *   f = the per-particle "Extra F" (functor_poisson_boltzmann_extra_f.h), added on every row whose kind has no bit of
 *       Solid (:79-81) -- Boundary rows included.  Any other row kind is an error.
 * J (functor_poisson_boltzmann_jacobian.h:38-108) = the Laplacian built once by isph_assemble_poisson_boltzmann (the
 * reference's A.is_filled), whose diagonal isph_pb_jacobian replaces: L_ii + kappa^2 g'(psi_i) on the Fluid-like rows
 * (the closed forms of :86-97), -1 on the Solid / Boundary rows, which hold no other (nonzero) entry.
 * Vectors cross this boundary in the caller's numbering with nlocal entries, as in isph_solve; ghost values of psi come
 * from the matrix' halo inside the SpMV.  The forward comm of psi after the solve (pair_isph.cpp:595-597) stays with
 * the caller (isph_halo_forward).  Non-convergence is reported in info, never an error.  With more than one rank the
 * residual, the solve and the preconditioner set-up are COLLECTIVE. */
typedef struct {
  double kappasq;           /* 2 ezcb / psiref (pair_isph.cpp:1680-1698; default 1)                         */
  double gamma;             /* steric "gamma" (0)                                                           */
  int linearized;           /* "linearized" (0)                                                             */
  int max_iters;            /* NOX::StatusTest::MaxIters (100)                                              */
  double f_tol;             /* NOX::StatusTest::NormF, unscaled 2-norm (1e-8)                               */
  double update_tol;        /* NOX::StatusTest::NormUpdate, unscaled 2-norm (1e-5); not met before step 1    */
  int prec_max_age;         /* "Preconditioner Reuse Policy" Reuse, "Max Age Of Prec" (10); 1 = every step   */
  int prec_kind;            /* 0 SA-AMG (ML in the reference's list), 1 block-Jacobi ILU(0)                 */
  isph_amg_params amg;      /* isph_amg_params_default                                                      */
  isph_solver_params linear;/* Block GMRES (flexible, right preconditioning), tol 1e-6, 80 iterations       */
  int prec_refresh;         /* 0 (default): at prec_max_age the preconditioner is destroyed and built again.  1: it is
                             * created while the pattern is held (as under isph_ctx_hold_pattern; the context's own
                             * setting is put back) and REFRESHED by isph_prec_refactor at prec_max_age -- J changes on
                             * its diagonal only, so the SA-AMG keeps the aggregates a fresh create would find -- where
                             * the type can be refactored (the ILU(0) blocks; the SA-AMG on one rank), rebuilt otherwise */
} isph_pb_params;
void isph_pb_params_default(isph_pb_params *p);
typedef struct {
  int status;               /* 1 converged, 0 MaxIters, -1 non-finite ||F|| (NOX FiniteValue)               */
  int newton_iters, linear_iters, prec_builds;   /* prec_builds counts a rebuild and a refresh alike */
  double norm_f, norm_update, ms;
  int prec_refreshes;       /* how many of prec_builds were refreshes (prec_refresh = 1)                     */
} isph_pb_info;
/* The Laplacian part of J, Laplacian(-1, eps) (FunctorOuterPoissonBoltzmannJacobian::enterFor, :47-68), -1 unit rows on
 * Solid / Boundary particles; psi0 [nall] the Dirichlet values (NULL: 0), eps [nall] the dielectric coefficient (NULL:
 * 1).  The matrix keeps its row classes, psi0, the positions of its diagonal entries and L_ii. */
int isph_assemble_poisson_boltzmann(isph_ctx *ctx, const isph_particles *P, int antisym, const double *eps /*[h|d]*/,
                                    const double *psi0 /*[h|d]*/, int ncol, isph_mat **J_out, int on_device);
/* computeF: F_out [nlocal] at psi [nlocal]; f [nlocal] or NULL.  Independent of the diagonal J holds. */
int isph_pb_residual(isph_ctx *ctx, const isph_mat *J, const isph_pb_params *prm, const double *psi, const double *f,
                     double *F_out, int on_device);
/* computeJacobian: J's diagonal at psi [nlocal], written in place */
int isph_pb_jacobian(isph_ctx *ctx, isph_mat *J, const isph_pb_params *prm, const double *psi, int on_device);
/* solveProblem: Newton from the caller's psi [nlocal] (the initial guess; updated in place), full step, constant forcing
 * term, FGMRES from x0 = 0 on J delta = -F with the preconditioner of prec_kind rebuilt when its age reaches
 * prec_max_age; stop on FiniteValue OR MaxIters OR (NormF AND NormUpdate) (solver_nox_impl.h:78-145,
 * solver_nox_stratimikos.h:84-122).  prm NULL: isph_pb_params_default. */
int isph_solve_poisson_boltzmann(isph_ctx *ctx, isph_mat *J, const isph_pb_params *prm, const double *f, double *psi,
                                 isph_pb_info *info, int on_device);

/* Particle shifting (fix isph/shift -> PairISPH_Corrected::shiftParticles, pair_isph_corrected.cpp:1203-1262).
 * isph_compute_shift replaces FunctorOuterComputeShift (functor_compute_shift.h:48-113): dr[nlocal][3] for the fluid
 * particles, pairs inside min(cutsq, shiftcut^2), alpha = shift*dt*vmax.
 * isph_apply_shift replaces FunctorOuterApplyShift (functor_apply_shift.h:76-108): p += grad p . dr,
 * v_k += grad v_k . dr, x += dr on the nlocal rows of x, v [nall][3], p [nall]; types with fixed[type] != 0
 * (PairISPH::isParticleFixed; fixed may be NULL) do not move.  All rows read the pre-shift state (the reference's
 * serial loop lets row i see rows < i already shifted).
 * isph_shift_particles is the whole shiftParticles(): vmax = max fluid |v| over all ranks (returned in *vmax_out
 * when not NULL), dr from shift*dt*vmax, then the apply. */
int isph_compute_shift(isph_ctx *ctx, const isph_particles *P, double alpha, double shiftcut, double nonfluidweight,
                       double *dr, int on_device);
int isph_apply_shift(isph_ctx *ctx, const isph_particles *P, int antisym, const int *fixed, const double *dr,
                     double *x, double *v, double *p, int on_device);
int isph_shift_particles(isph_ctx *ctx, const isph_particles *P, int antisym, const int *fixed, double shift,
                         double shiftcut, double nonfluidweight, double dt, double *x, double *v, double *p,
                         double *vmax_out, int on_device);

/* ---- two-phase flow: wall normals and surface tension ------------------- */

/* PairISPH_Corrected::computeNormals for boundary_particle == Solid without use_part (ref: pair_isph_corrected.cpp:
 * 374-425) -> Corrected::FunctorOuterNormal (functor_normal.h:57-133), both of its passes ((Fluid, Solid) and (Solid,
 * Fluid), orientation -1 on Fluid / buffer particles and +1 on Solid ones, :381-386) in one neighbour sweep: unit
 * normals normal_out [nlocal][3] (zero where a particle has no neighbour of the opposite kind, and on other kinds) and,
 * when pnd_out is not NULL, the particle number density of isph_compute_pnd [nlocal].  Needs P->Gc and P->vfrac.
 * Ghost values are the caller's forward comm.  bd_coord (functor_normal.h:138-191) and use_part are not provided. */
int isph_compute_normals(isph_ctx *ctx, const isph_particles *P, double *normal_out, double *pnd_out, int on_device);

/* st.csf of the reference: color 0 Corrected / 1 Adami ("Color Gradient", color.h:28-66), alpha, theta (contact
 * angle of phase 1; pi - theta for the others), epsilon (in-phase volume-ratio cut-off), kappa; defaults 1, 0, 0.01,
 * 100 (pair_isph.cpp:1583-1586).  phase: [ntypes+1] getParticlePhase(type) (pair_isph.cpp:169), host always,
 * solids 0. */
typedef struct {
  int color;
  double alpha, theta, epsilon, kappa;
  const int *phase;
} isph_csf_params;
void isph_csf_params_default(isph_csf_params *p);

/* PairISPH_Corrected::computeSurfaceTension_ContinuumSurfaceForce (ref: pair_isph_corrected.cpp:684-758) as two
 * neighbour sweeps.  Both need P->Gc and P->vfrac and the filter (Fluid, Fluid).
 *
 * isph_csf_phase_normal = FunctorOuterPhaseGradient (functor_phase_gradient.h:49-141) + FunctorOuterNormalizeVector
 * (functor_normalize_vector.h:29-41) + FunctorOuterCorrectPhaseNormal (functor_correct_phase_normal.h:43-95, only when
 * wall_normal is given; reads P->pnd): nmag_out [nlocal][4] = {n_x, n_y, n_z, |grad c|} (32-byte aligned when on the
 * device), grad_out [nlocal][3] the gradient before normalisation (may be NULL).  rho [nall] or NULL (= 1);
 * wall_normal = pair->normal, owned rows read.
 *
 * isph_csf_force = FunctorOuterPhaseDivergence (functor_phase_divergence.h:41-98) + FunctorOuterContinuumSurfaceForce
 * (functor_continuum_surface_force.h:52-64): nmag [nall][4] with the ghost records filled (the reference's forward
 * comms of work3 / work), f_inout [nlocal][3] receives -= alpha (1 - exp(-kappa/|kappa_i|)) kappa_i n_i mag_i,
 * kappa_out [nlocal] the curvature (may be NULL).  DEPARTURE: an active particle whose curvature is exactly 0 adds
 * nothing; the reference computes alpha (1 - exp(+inf)) 0 = NaN there (:58-62), which on an exact lattice is a matter
 * of summation order on every flat interface.
 *
 * isph_surface_tension_csf = both sweeps; ghost records are read through P->colmap (an image of an owned particle
 * reads its owner), off-rank ghosts (colmap >= nlocal) through one isph_halo_forward of the records when plan is not
 * NULL (with plan == NULL every ghost must be such an image).  nmag_out [nlocal][4] or NULL. */
int isph_csf_phase_normal(isph_ctx *ctx, const isph_particles *P, const isph_csf_params *prm, const double *rho,
                          const double *wall_normal, double *grad_out, double *nmag_out, int on_device);
int isph_csf_force(isph_ctx *ctx, const isph_particles *P, const isph_csf_params *prm, const double *nmag,
                   double *f_inout, double *kappa_out, int on_device);
int isph_surface_tension_csf(isph_ctx *ctx, const isph_particles *P, const isph_csf_params *prm,
                             const isph_halo_plan *plan, const double *rho, const double *wall_normal, double *f_inout,
                             double *nmag_out, int on_device);

/* PairISPH_Corrected::computeSurfaceTension_PairwiseForce (ref: pair_isph_corrected.cpp:760-784) ->
 * FunctorOuterPairwiseForce (functor_pairwise_force.h:31-83), filter (Fluid, Fluid):
 * f_i += sum_j -F(s[phase_i][phase_j], r, sqrt(cutsq)) r_ij / r with model 0 TartakovskyMeakin, 1 / 2
 * TartakovskyPanchenko Var1 / Var2 (pairwise_force.h:38-118).  phase [ntypes+1] and s [nphase][nphase] are host
 * arrays; f_sum (host, may be NULL) receives this rank's sum of the added forces, the functor's _f_sum. */
int isph_pairwise_force(isph_ctx *ctx, const isph_particles *P, int model, const int *phase, const double *s,
                        int nphase, double *f_inout, double f_sum[3], int on_device);

/* ---- body forces: electrostatic force and random stress ------------------ */

/* FunctorOuterSmoothField, scalar form (functor_smooth_field.h:43-106): sf_i = f_i W(0,h_ii) V_i + sum_j f_j W(r_ij) V_j,
 * with FilterBinary(filt_i, filt_j) when use_filter.  f [nall], sf_out [nlocal].  One pass.  Rows whose kind fails the
 * filter are NOT written (the functor returns first): they keep what sf_out held.  Needs P->vfrac [nall].
 *
 * The smoothing loop of computeAppliedElectricPotential (pair_isph_corrected.cpp:576-593, ae.smooth_phi passes over the
 * conductivity that feeds isph_assemble_applied_potential) is the caller's to write.  That loop copies only nlocal
 * entries of the result back into its input sigmatmp and communicates `work`, not sigmatmp: from the second pass on the
 * reference still reads the UNSMOOTHED ghost values.  This entry point is one pass, and the caller decides what the
 * ghosts of f hold (its own forward comm of the previous pass, or the reference's stale values). */
int isph_smooth_field(isph_ctx *ctx, const isph_particles *P, const double *f /*[nall]*/, int use_filter, int filt_i,
                      int filt_j, double *sf_out /*[nlocal]*/, int on_device);

typedef struct {
  double ezcb, psiref, gamma;   /* pb.ezcb, pb.psiref, pb.gamma: 0, 1, 0 (pair_isph.cpp:1684-1698) */
  double pb_e[3];               /* pb.e: the field used when phi == NULL                           */
  double ae_e[3];               /* ae.e: phigrad = -ae_e on the buffer rows                        */
} isph_ek_params;
void isph_ek_params_default(isph_ek_params *p);

/* computePsiGradient + computePhiGradient + computeElectrostaticForce in ONE neighbour sweep.
 *
 * psi gradient = Corrected::FunctorOuterGradient (functor_gradient.h:80-169) with FilterBinary(Fluid, All)
 * (pair_isph_corrected.cpp:540-565).  The reference's call sites use the Symmetric family (default template argument,
 * :551-558): antisym = 0 needs P->Gc; antisym = 1 is offered as everywhere else in this ABI.  When P->morris_holmes is
 * set, a pair whose i is not Solid and whose j is Solid is weighted by MirrorMorrisHolmes::computeMirrorCoefficient(
 * sqrt(cutsq)) (functor_boundary_morris_holmes.h:99-102, mirror_morris_holmes.h:39-52): needs P->pnd and P->vfrac, both
 * [nall].  Rows that fail the filter hold exact zeros (the memset at :544).
 *
 * phi gradient (only when phi != NULL; phigrad_out is not touched otherwise) = the same functor with
 * FilterBinary(Fluid, Fluid) and MirrorNothing; afterwards the rows whose kind is exactly BufferDirichlet or
 * BufferNeumann hold -ae_e in all three components (pair_isph_corrected.cpp:621-651).  Fluid = 99 contains the buffer
 * bits, so buffer rows do pass the filter first; the override decides their value.
 *
 * force on EVERY owned particle, no filter (functor_electrostatic_force.h:39-56, pair_isph.cpp:679-687):
 *   f_i[k] -= ezcb 2 sinh(psi_i) / (1 + 2 gamma sinh^2(psi_i / 2)) (-psiref d_k psi_i + e_k),  k < dim,
 * e = -grad phi_i (after the override) when phi is given, else pb_e.  The functor uses sinh also when the
 * Poisson-Boltzmann solve was linearized; so does this.
 *
 * psi, phi [nall] with ghosts filled; psigrad_out, phigrad_out [nlocal][3] or NULL; f_inout [nlocal][3], or NULL for the
 * gradients alone. */
int isph_electrostatic_force(isph_ctx *ctx, const isph_particles *P, int antisym, const isph_ek_params *prm,
                             const double *psi /*[nall]*/, const double *phi /*[nall] or NULL*/,
                             double *psigrad_out /*[nlocal][3] or NULL*/, double *phigrad_out /*[nlocal][3] or NULL*/,
                             double *f_inout /*[nlocal][3] or NULL: gradients only*/, int on_device);

/* ns.is_fluctuation_enabled -> computeForceFromRandomStress (pair_isph_corrected.cpp:130-132, 812-826).
 *
 * isph_random_stress_tensor = computeRandomStressTensor (pair_isph.cpp:710-758) on the owned rows with kind & Fluid:
 * dim^2 standard normals g, R[k2][k1] = g[k2 dim + k1], T = (R + R^T) / 2, T[k][k] -= tr T / dim; other rows hold
 * zeros.  rs_out [nlocal][6] = T packed as (0,0), (0,1), (1,1), (0,2), (1,2), (2,2), the order of Lc (48 bytes per ghost
 * record instead of the 72 of the reference's three [nmax][3] arrays; in 2-D the last three are zero), 16-byte aligned
 * when on the device.  tag [nlocal] = atom->tag.
 *
 * DEPARTURE: the reference draws from LAMMPS' per-rank RanMars stream in ilist order, so its numbers depend on the
 * decomposition and the atom order.  Here the normals are a pure function of (seed, step, tag): Philox4x32-10 with
 * key = (seed low 32, seed high 32) and counter = (tag, b, step low, step high) for the draw block b = 0..1 (2-D) or
 * 0..4 (3-D); the outputs (o0, o1, o2, o3) give u1 = (((o0 2^32 + o1) >> 11) + 0.5) 2^-53 and u2 likewise from (o2, o3);
 * g[2b] = sqrt(-2 ln u1) cos(2 pi u2), g[2b+1] = sqrt(-2 ln u1) sin(2 pi u2); the tenth normal in 3-D is dropped.  The
 * same particle gets the same tensor on any rank count and in any atom order.
 *
 * isph_random_stress_force = FunctorOuterRandomStress with FunctorOuterDivergenceAntiSymmetric
 * (functor_random_stress.h:54-74) on the rows with kind & Fluid, pairs FilterBinary(Fluid, Fluid):
 *   d_c = -sum_j r_ij . (T_i[:,c] + T_j[:,c]) W'/r sqrt(V_i V_j),   f_i[c] += d_c sqrt(2 kBT nu_i rho_i / dt / V_i),
 * all dim columns from one sweep (the reference makes three functor calls per particle).  rs [nall][6] with the ghost
 * records filled; nu, rho [nlocal]; does not read Gc.
 *
 * isph_force_from_random_stress = tensors + ghost fill + sweep; ghost records are read through P->colmap (an image of an
 * owned particle reads its owner), off-rank ghosts (colmap >= nlocal) through one isph_halo_forward of the 6-double
 * records when plan is not NULL.  rs_out [nlocal][6] or NULL. */
int isph_random_stress_tensor(isph_ctx *ctx, const isph_particles *P, const int *tag /*[nlocal]*/,
                              unsigned long long seed, unsigned long long step,
                              double *rs_out /*[nlocal][6]*/, int on_device);
int isph_random_stress_force(isph_ctx *ctx, const isph_particles *P, double dt, double kBT, const double *nu /*[nlocal]*/,
                             const double *rho /*[nlocal]*/, const double *rs /*[nall][6], ghosts filled*/,
                             double *f_inout /*[nlocal][3]*/, int on_device);
int isph_force_from_random_stress(isph_ctx *ctx, const isph_particles *P, const isph_halo_plan *plan, const int *tag,
                                  unsigned long long seed, unsigned long long step, double dt, double kBT,
                                  const double *nu, const double *rho, double *f_inout,
                                  double *rs_out /*[nlocal][6] or NULL*/, int on_device);

/* ---- ghost atoms and the full neighbour list ----------------------------- */

/* What LAMMPS does between two calls of PairISPH::compute when the particles have moved, for ONE rank: wrap into the box,
 * create the ghost atoms (periodic images within the cut of a face) and rebuild the full neighbour list (Neighbor::build).
 * The device twin of isph_cloud_build (isph_workload.h): for a fully periodic box with lo = 0 the result equals it bit for
 * bit -- the same ghosts in the same order, the same positions, owners, offsets and list entries.
 *
 *   wrap (periodic axes, wrap != 0)   t = x - lo, P = hi - lo: r = fmod(t, P); r < 0: r += P; r >= P: r = 0; x = r + lo
 *   images  on a periodic axis a shift +1 when x_a - lo_a < cut, -1 when x_a >= hi_a - cut; every non-zero combination of
 *           the shifts, z outermost and x innermost, ascending, owners ascending; position x_a + s_a P_a (z = 0 in 2-D)
 *   list    j != i with ((d0 d0) + d1 d1) + d2 d2 < cut cut, every product and sum rounded (no fused multiply-add);
 *           every row in ascending particle index; offsets in the CSR form of isph_particles
 *
 * A non-periodic axis gets no wrap and no images.  Off-rank ghosts (LAMMPS' Comm): isph_nlist_build_dist below.  Every device buffer
 * comes from the library's pool; only the two counts (ghosts, list entries) are read back during the build. */
typedef struct isph_nlist isph_nlist;

/* x: [nlocal][3] [h|d].  lo/hi/periodic: the caller's box (LAMMPS domain->boxlo/boxhi/periodicity).
 * wrap != 0: owned positions are first wrapped into [lo, hi) on periodic axes.
 * cut: one radius (the caller passes its largest pair cut + skin).
 * Fails (-1, isph_last_error) for dim not 2|3, cut <= 0, or a periodic axis shorter than 2 cut. */
int isph_nlist_build(isph_ctx *ctx, int dim, int nlocal, const double *x,
                     const double lo[3], const double hi[3], const int periodic[3],
                     double cut, int wrap, int on_device, isph_nlist **out);

/* info: [0] nlocal  [1] nghost  [2] list entries  [3] 1 when the entries fit 32-bit offsets (fewer than 2^31 - 1) */
int isph_nlist_info(const isph_nlist *nl, long long info[4]);

/* copies out; any pointer may be NULL; neigh_ptr (32-bit) only when info[3]; all [h|d] per on_device.
 * x_all [nall][3], owner_index [nall], neigh_ptr64 / neigh_ptr [nlocal + 1], neigh_idx [entries].
 * isph_ctx_hold_neighbours is keyed on the caller's list arrays: a caller that copies a rebuilt list into the arrays of the
 * list before must drop the hold first (isph_ctx_hold_neighbours(ctx, 0)), or the operators keep reading the old layout. */
int isph_nlist_get(isph_ctx *ctx, const isph_nlist *nl, double *x_all, int *owner_index,
                   long long *neigh_ptr64, int *neigh_ptr, int *neigh_idx, int on_device);

int isph_nlist_destroy(isph_ctx *ctx, isph_nlist *nl);

/* ---- the same step on a brick of ranks: migration, off-rank ghosts, list, column map, halo plan --------------------- */

/* What LAMMPS' Comm (exchange, borders, forward_comm) and Neighbor::build do between two compute() calls on several
 * ranks, and what Epetra's FillComplete derives from the result (column map + Import), on the device.  Everything between
 * ranks goes through the context's communicator (RCCL or the host-staged callbacks): point-to-point exchanges with the
 * at most 26 grid neighbours and max all-reduces of a failure flag.  Integers travel as doubles.  Every call of this
 * section is COLLECTIVE: every rank of the context makes it, with the same decomposition, cut and prune; a rank that
 * fails a check of its own carries the failure to the next consensus, where all ranks fail together (the others with
 * "... failed on another rank").  One rank without a communicator is allowed.
 *
 * The decomposition: a grid of pgrid[0] x pgrid[1] x pgrid[2] sub-boxes cut by planes; grid cell c of axis a owns x
 * (after the wrap of isph_nlist_build on periodic axes) when faces[a][c] <= x < faces[a][c + 1] -- a particle on a face
 * belongs to the upper cell.  Beyond a non-periodic outer face the outer cell owns. */
typedef struct {
  int dim;                 /* 2 | 3 */
  double lo[3], hi[3];     /* the global box */
  int periodic[3];
  int pgrid[3];            /* ranks per axis; rank = cx + pgrid[0] * (cy + pgrid[1] * cz) */
  const double *faces[3];  /* faces[a][0 .. pgrid[a]]: cut planes, faces[a][0] = lo, last = hi; NULL: uniform,
                              lo + c * ((hi - lo) / pgrid[a]), the last one hi itself (host always) */
} isph_decomp;

/* Ghosts, list, column map and halo plan of this rank's nlocal owned particles x [nlocal][3] [h|d] (nlocal = 0 takes
 * part).  Refused by name: pgrid[0] * pgrid[1] * pgrid[2] != the context's rank count; a sub-box narrower than cut on an
 * axis with more than one rank; a periodic axis with one rank shorter than 2 cut; owned particles outside the rank's
 * sub-box after the wrap (the message carries their number).
 *
 *   border  on axis a a particle is needed on the low side when x_a - flo_a < cut and on the high side when
 *           x_a >= fhi_a - cut (flo / fhi: the owner's faces); every non-zero combination over the axes; nothing crosses a
 *           non-periodic outer face; the receiver is the rank at that grid offset, wrapped on periodic axes; the image
 *           shift s_a in {-1, 0, +1} is non-zero exactly when the offset crosses the periodic boundary (to the low side
 *           from grid coordinate 0: +1); position x_a + s_a P_a, rounded once, z = 0 in 2-D.  An axis with one rank gives
 *           the self-images of isph_nlist_build.
 *   ghosts  follow the owned particles, sorted by owner rank, owner index, shift (sz outermost, sx innermost), ascending;
 *           this rank's own images stand at its own rank's place.  With two ranks on a periodic axis a particle may arrive
 *           twice with different shifts: two ghosts, one column.  On one rank everything equals isph_nlist_build bit for bit.
 *   list    as isph_nlist_build, over owned + ghost particles.
 *   prune   != 0: the ghosts no owned row lists are dropped (Epetra's column map holds inserted columns only), neigh_idx
 *           is renumbered, and the senders learn which of their particles survived.
 *   colmap  owned i -> i; a self-image -> its owner's index; an off-rank ghost -> nlocal + the rank of its (owner rank,
 *           owner index) among the distinct such pairs, ascending.
 *   plan    peers: the ascending ranks with traffic in either direction; send_idx per peer: the ascending distinct owned
 *           indices that peer holds; recv_ptr: the ghost columns per peer (isph_mat_set_halo / isph_halo_create take them).
 *
 * Read back during a build: the record counts per neighbour rank (each way), the ghost, column and send counts per
 * neighbour rank, the number of list entries, the consensus flags.  Device buffers come from the library's pool.
 * isph_nlist_info / isph_nlist_get / isph_nlist_destroy work on the result; owner_index is the index on the owner's rank. */
int isph_nlist_build_dist(isph_ctx *ctx, const isph_decomp *dc, int nlocal, const double *x, double cut, int prune,
                          int on_device, isph_nlist **out);

/* info: [0] nlocal  [1] nghost  [2] list entries  [3] fits32  [4] ncol (owned + ghost columns)  [5] npeers
 *       [6] send entries  [7] off-rank ghosts */
int isph_nlist_dist_info(const isph_nlist *nl, long long info[8]);

/* copies out; any pointer may be NULL; [h|d] per on_device.  owner_rank / colmap [nall], peers [npeers],
 * send_ptr / recv_ptr [npeers + 1], send_idx [send entries]. */
int isph_nlist_dist_get(isph_ctx *ctx, const isph_nlist *nl, int *owner_rank, int *colmap, int *peers, int *send_ptr,
                        int *send_idx, int *recv_ptr, int on_device);

/* forward_comm_pair of a per-atom array a [nall][ncomp] [h|d], in place: rows >= nlocal receive their owner's row, from
 * this rank (self-images) or through one exchange of the distinct ghost columns over the list's plan.  Collective. */
int isph_nlist_forward(isph_ctx *ctx, const isph_nlist *nl, int ncomp, double *a, int on_device);
int isph_nlist_forward_int(isph_ctx *ctx, const isph_nlist *nl, int ncomp, int *a, int on_device);
/* The forward comm of up to 8 per-atom arrays in ONE exchange, as PairISPH::pack_forward_comm sends several fields per
 * message: a record of sum(ncomp) doubles per listed atom, ints travelling as doubles.  arr[j].a is [nall][ncomp] doubles,
 * or ints when is_int != 0, [h|d] per on_device, updated in place.  The result equals narrays single forwards bit for
 * bit.  Collective: the arguments are checked before a consensus (one max all-reduce) that stands before the exchange,
 * so a rank whose arguments are refused fails its peers with it ("... failed on another rank"). */
typedef struct {
  void *a;
  int ncomp;
  int is_int;
} isph_fwd_array;
int isph_nlist_forward_multi(isph_ctx *ctx, const isph_nlist *nl, int narrays, const isph_fwd_array *arr, int on_device);

/* Comm::exchange: the positions x [nlocal][3] are wrapped; a particle whose wrapped position lies in another sub-box goes
 * to that rank with its nd doubles fd [nlocal][nd] and ni ints fi [nlocal][ni] (either may be 0 / NULL).  The target must
 * be one of the 26 (8 in 2-D) grid neighbours, else ALL ranks fail with "moved farther than one sub-box".  New owned
 * order: the stayers in their old order, then the arrivals sorted by (source rank, source index).  Collective. */
typedef struct isph_migrated isph_migrated;
int isph_migrate(isph_ctx *ctx, const isph_decomp *dc, int nlocal, const double *x, int nd, const double *fd, int ni,
                 const int *fi, int on_device, isph_migrated **out);
/* info: [0] the new nlocal  [1] particles sent  [2] particles received */
int isph_migrated_info(const isph_migrated *mg, long long info[3]);
/* x [nlocal'][3], fd [nlocal'][nd], fi [nlocal'][ni]; any pointer may be NULL; [h|d] per on_device */
int isph_migrated_get(isph_ctx *ctx, const isph_migrated *mg, double *x, double *fd, int *fi, int on_device);
int isph_migrated_destroy(isph_ctx *ctx, isph_migrated *mg);

/* ---- the glue of a time step: ghost rows, zero-mean pressure, observables ----------------------------------------- */

/* What a time step needs between the neighbour sweeps, and the numbers the reference's scripts record, for ONE rank: isph_ghost_fill,
 * isph_zero_mean_pressure, isph_status and isph_tgv_error refuse a context with a communicator (isph_ctx_create_dist /
 * _hostcomm) by name; the forms over several ranks are isph_nlist_forward and the three *_dist entry points below.  All
 * pointers [h|d] per on_device unless marked host; work buffers come from the library's pool; everything runs on the
 * context's stream.  The sums are two-stage reductions over a partition that depends on the row count alone, summed in a
 * fixed order, without floating-point atomics (the discipline of the solvers' multi-dot): the bits of a result do not
 * change from run to run.
 *
 * isph_ghost_fill: forward_comm_pair for the periodic images of one rank (what PairISPH::pack_forward_comm /
 * unpack_forward_comm do through Comm when every ghost is an image of an owned atom, pair_isph.cpp:1924-2125):
 * row i >= nlocal of a [nall][ncomp] receives row owner[i], in place.  Any ncomp >= 1.  nall == nlocal launches nothing
 * (owner and a may then be NULL).  An owner[i] outside [0, nlocal) anywhere fails the call -- checked on the device, one
 * flag is read back; the rows of valid owners may have been written by then. */
int isph_ghost_fill(isph_ctx *ctx, int nlocal, int nall, const int *owner /*[nall]*/, int ncomp,
                    double *a /*[nall][ncomp], in place*/, int on_device);

/* PairISPH::computeZeroMeanPressure (ref: pair_isph.cpp:422-464).  Owned rows whose kind is exactly Solid (12) are set
 * to 0, whatever they held, and left out; mean = sum / count over the other owned rows; with update != 0 the mean is
 * subtracted from all nall entries whose kind is not Solid (ghost Solid rows are left as they are).  kind: [ntypes + 1],
 * host always, as in isph_particles.  The mean stays on the device between the kernels and is read back only when
 * mean_out (host) is not NULL.
 * Departure: a count of 0 gives mean 0 and subtracts nothing (the reference divides by zero there). */
int isph_zero_mean_pressure(isph_ctx *ctx, int nlocal, int nall, const int *type /*[nall]*/, const int *kind /*[h]*/,
                            int ntypes, double *f /*[nall], in place*/, int update, double *mean_out /*host, may be NULL*/,
                            int on_device);

/* ComputeISPH_Status::compute_vector (ref: compute_isph_status.cpp:141-175) over the owned rows with
 * type_mask & (1 << (type - 1)), in one sweep: out = { count, sum vx, sum vy, sum vz, sum V, sum rho V,
 * sum 1/2 rho V |v|^2, max |v| } with V = P->vfrac (required); the maximum is taken over the rows within `radius` of
 * `centre`, and only when radius > 0 (0 otherwise).  Of P only nlocal, x, type and vfrac are read.  Every term is formed
 * with the roundings of the reference's loop (no fused multiply-add); out is a host array. */
int isph_status(isph_ctx *ctx, const isph_particles *P, int type_mask, const double *v /*[nlocal][3]*/,
                const double *rho /*[nlocal]*/, const double centre[3] /*host*/, double radius, double out[8] /*host*/,
                int on_device);

/* FixISPH_TGV::compute_error (ref: fix_isph_tgv.cpp:76-116) for the 2-D Taylor-Green vortex at time t with amplitude
 * umax: out = { pressure l2 error, pressure norm, velocity l2 error, velocity norm }, each sqrt(sum / nlocal).  The
 * mean of p over all owned rows is removed from the pressure error as the reference removes it (the exact field has
 * mean 0); the exact velocity has no z component.  x, vnp1: [nlocal][3]; p, rho, nu: [nlocal]; out is a host array.
 * The ALE start-up branch of the reference (:93-97, which overwrites the state) is not provided. */
int isph_tgv_error(isph_ctx *ctx, int nlocal, int dim, const double *x, const double *vnp1, const double *p,
                   const double *rho, const double *nu, double t, double umax, double out[4] /*host*/, int on_device);

/* The same three over the ranks of the context's communicator.  COLLECTIVE: every rank calls, nlocal = 0 takes part; a
 * context with RCCL, with the host-staged transport, or without a communicator is accepted.  A rank whose arguments are
 * refused fails the others with it ("... failed on another rank") at a consensus that stands before the first all-reduce.
 *   isph_zero_mean_pressure_dist  sum and count over the owned non-Solid rows of ALL ranks (one sum all-reduce); owned
 *                                 Solid rows are zeroed; the mean is subtracted from all nall non-Solid entries of this
 *                                 rank; a count of 0 over all ranks gives mean 0.
 *   isph_status_dist              the seven sums (one sum all-reduce) and the maximum (one max all-reduce) over all ranks.
 *   isph_tgv_error_dist           the pressure mean over the owned rows of all ranks first, then the four sums (two sum
 *                                 all-reduces), then sqrt(sum / N) with N the rows of all ranks.
 * The reduction: the two-stage fixed-order reduction per rank, whose result goes into the rank's slot of an nranks-wide
 * device vector that is otherwise 0; the sum all-reduce adds the vectors -- adding zeros is exact, so every slot arrives
 * with the bits its rank computed --; a small kernel adds the slots in rank order.  So the bits of a result are the same
 * on every rank, from run to run and from transport to transport; they differ from the result of another rank count by
 * round-off only; without a communicator they are the bits of the one-rank entry point. */
int isph_zero_mean_pressure_dist(isph_ctx *ctx, int nlocal, int nall, const int *type /*[nall]*/, const int *kind /*[h]*/,
                                 int ntypes, double *f /*[nall], in place*/, int update,
                                 double *mean_out /*host, may be NULL*/, int on_device);
int isph_status_dist(isph_ctx *ctx, const isph_particles *P, int type_mask, const double *v /*[nlocal][3]*/,
                     const double *rho /*[nlocal]*/, const double centre[3] /*host*/, double radius,
                     double out[8] /*host*/, int on_device);
int isph_tgv_error_dist(isph_ctx *ctx, int nlocal, int dim, const double *x, const double *vnp1, const double *p,
                        const double *rho, const double *nu, double t, double umax, double out[4] /*host*/,
                        int on_device);

/* ---- the time step of incompressible Navier-Stokes, resident on the device ------------------------------------------ */

/* An isph_ins owns ONE rank's state on the device -- x, v, vstar, the force f and the wall normals [nall][3]; p, dp, rho,
 * nu, vfrac, pnd, type [nall]; Gc, Lc [nlocal][.]; the owner map and the full neighbour list -- and chains the entry
 * points above into the phases of the reference:
 *
 *   PairISPH::compute (pair_isph.cpp:1241-1380)          isph_ins_pre  (computePre, body-force reset)
 *                                                        [the caller's forces through isph_ins_view / isph_ins_force]
 *                                                        isph_ins_solve (computeIncompressibleNavierStokes, :910-1034)
 *   FixISPH::final_integrate -> advanceTime              isph_ins_advance (pair_isph_corrected.cpp:1172-1199)
 *   FixISPH_Shift::final_integrate                       isph_ins_shift   (fix_isph_shift.cpp:146-163)
 *   LAMMPS between two compute() calls                   isph_ins_set_list (the caller's) or isph_ins_rebuild
 *
 * Every neighbour sweep, assembly and solve is the call a user of this header would make with device operands; the glue
 * is isph_ghost_fill, isph_zero_mean_pressure and two transposes.  During a step only what those calls read back is
 * read back: the two counts of a list build, the solve infos, the shift's vmax; the owner map is validated once when a
 * list is taken; the zero-mean value stays on the device.
 *
 * Out of scope, refused by name: a context with a communicator (isph_ins_create is one rank; isph_ins_create_dist at the
 * end of this section runs the same phases on a brick of ranks); block Helmholtz
 * (isph_assemble_block_helmholtz / isph_solve_block); the MorrisHolmes boundary; bd_coord and use_part wall normals; a
 * recycle handle; a context in hold-pattern mode (isph_ctx_hold_pattern).  Solid particles need antisym = 0 (the wall
 * normals read Gc).
 * Departures: isph_zero_mean_pressure's (count 0); G and L are not formed for antisym = 1, which never reads them (the
 * reference's computePre forms them always); the shift's fixed types are those of kind Solid.
 * Call isph_ins_params_default FIRST and then change fields: the struct grows at its tail.  The tables and the strings
 * are copied by isph_ins_create. */
typedef struct isph_ins isph_ins;
typedef struct {
  int dim;                   /* 2 | 3 (default 3)                                                                    */
  int kernel;                /* 0 Wendland, 1 Quintic, 2 Cubic                                                       */
  int antisym;               /* 1 = the momentum-preserving family (default), 0 = the corrected one                  */
  double theta;              /* ns.theta (default 0.5); |theta| < 1e-24: the Helmholtz right-hand side is the result  */
  double dt;                 /* time step; required                                                                  */
  int incremental_pressure;  /* ns.is_incremental_pressure_used (default 1)                                          */
  int singular_mode;         /* 0 NotSingular, 1 NullSpace (default), 2 PinZero, 3 DoubleDiag                        */
  double g[3];               /* gravity                                                                              */
  int ntypes;                /* host tables as in isph_particles: kind [ntypes+1], h and cutsq [(ntypes+1)^2]        */
  const int *kind;
  const double *h, *cutsq;
  const char *prec_helmholtz;   /* a type string of isph_prec_create (default "bjacobi-ilu0") ...                     */
  int helmholtz_block_size;     /* ... and its block_size (default 512)                                               */
  const char *prec_poisson;     /* the same for the Poisson solve; "sa-amg" on a NullSpace system gets the normalised  */
  int poisson_block_size;       /* null mask as its null vector (isph_prec_create_amg)                                 */
  isph_solver_params solver;    /* both solves                                                                        */
  double lo[3], hi[3];          /* the box of isph_ins_rebuild (isph_nlist_build) ...                                 */
  int periodic[3];
  double cut;                   /* ... and its list radius; 0 (default): isph_ins_rebuild is not available            */
  double shift, shiftcut, nonfluidweight;  /* fix isph/shift; shift = 0 (default): isph_ins_run does not shift        */
  int block_helmholtz, morris_holmes, normals_bd_coord, normals_use_part;  /* out of scope: non-zero is refused        */
  const void *recycle;                                                     /* out of scope: non-NULL is refused        */
  double tgv_umax;              /* the diagnostics of isph_ins_run: umax of isph_tgv_error (default 0.1) ...          */
  int status_type_mask;         /* ... and type_mask (default -1: every type), centre, radius of isph_status          */
  double status_centre[3], status_radius;
} isph_ins_params;
void isph_ins_params_default(isph_ins_params *p);
typedef struct {
  isph_solve_info helmholtz, poisson;   /* helmholtz.converged = 1 and 0 iterations when theta = 0 (no solve) */
} isph_ins_info;

int isph_ins_create(isph_ctx *ctx, const isph_ins_params *prm, isph_ins **S);
void isph_ins_destroy(isph_ins *S);
/* x, v [nlocal][3]; p, rho, nu, type [nlocal] of the owned particles, [h|d].  Drops the list.  The null mask of the
 * Poisson solve, !(kind & Solid), is made here (a host array, because isph_solve takes it from the host): with device
 * operands `type` is copied back once. */
int isph_ins_set_state(isph_ins *S, int nlocal, const double *x, const double *v, const double *p, const int *type,
                       const double *rho, const double *nu, int on_device);
/* The caller's ghosts and full list, what LAMMPS hands to PairISPH::compute: x_all [nall][3] (rows >= nlocal are read),
 * owner [nall] (periodic images of owned atoms only), neigh_ptr [nlocal+1] or neigh_ptr64 (one may be NULL), neigh_idx;
 * all copied.  v, p, rho, nu and type of the ghosts are gathered through the owner map. */
int isph_ins_set_list(isph_ins *S, int nall, const double *x_all, const int *owner, const int *neigh_ptr,
                      const long long *neigh_ptr64, const int *neigh_idx, int on_device);
/* Ghosts and list from the owned positions with isph_nlist_build (wrap on); the positions never leave the device. */
int isph_ins_rebuild(isph_ins *S);
/* info: [0] nlocal [1] nall [2] list entries (-1: no list) [3] steps isph_ins_run has completed [4] 1 between
 * isph_ins_pre and the next move [5] 1 when a Solid particle is present */
int isph_ins_sizes(const isph_ins *S, long long info[6]);
/* Copies a field out, [h|d]: "x" "v" "vstar" "f" "normal" ([.][3]), "p" "dp" "rho" "nu" "vfrac" "pnd" ([.]), "Gc"
 * ([nlocal][dim*dim]) "Lc" ([nlocal][dimL]), "type" "owner" (int); nlocal rows, or nall with with_ghosts. */
int isph_ins_get(isph_ins *S, const char *name, int with_ghosts, void *out, int on_device);
/* computePre (pair_isph_corrected.cpp:302-313): holds the neighbour layout for the step (isph_ctx_hold_neighbours),
 * volumes and their ghosts, G and L unless antisym, wall normals and pnd (isph_compute_normals) when a Solid kind is
 * present, f = 0.  Fails without a list.  The hold is the driver's from here on: taking a new list, isph_ins_set_state and
 * isph_ins_destroy release it, so a caller does not hold the layout of the same context for lists of its own meanwhile. */
int isph_ins_pre(isph_ins *S);
/* After isph_ins_pre: the particle view of the state (device pointers, valid until the next list) and the force
 * [nall][3] the Helmholtz right-hand side reads -- the caller adds surface tension, electrostatic force or random stress
 * with the entry points above, where the reference adds to atom->f. */
int isph_ins_view(const isph_ins *S, isph_particles *P);
double *isph_ins_force(isph_ins *S);
/* f [rows][3] [h|d], rows = nlocal or nall, is added to that force: for callers that hold a force of their own. */
int isph_ins_add_force(isph_ins *S, int rows, const double *f, int on_device);
/* computeIncompressibleNavierStokes (pair_isph.cpp:910-1034): Helmholtz assembly with x0 = v and the dim-column solve
 * (theta = 0: the right-hand side is copied); vstar with its ghosts (one kernel); Poisson assembly in singular_mode, wall
 * Neumann rows from the normals; the solve from zero with the null mask when NullSpace; ghosts of dp; zero-mean pressure
 * when incremental; isph_correct_velocity_pressure; ghosts of the corrected vstar.  Preconditioners are built and
 * destroyed around each solve, as the reference does.  Non-convergence is reported in info, not an error.  Fails before
 * isph_ins_pre. */
int isph_ins_solve(isph_ins *S, isph_ins_info *info /*may be NULL*/);
/* advanceTime: isph_advance_begin, the ghosts of its dp, isph_advance_end over owned particles AND ghosts (as
 * functor_advance_time_end.h:36-72 does), so a ghost moves with its owner. */
int isph_ins_advance(isph_ins *S);
/* FixISPH_Shift::final_integrate: computePre on the moved particles with the list of the step (volumes; G and L unless
 * antisym), then isph_shift_particles; vmax_out (host, may be NULL) = the max fluid speed it used. */
int isph_ins_shift(isph_ins *S, double *vmax_out);
/* out[0..3] = isph_tgv_error of (x, vstar, p) at time t, out[4..11] = isph_status of (x, vstar, rho, vfrac): the numbers
 * fix isph/tgv and compute isph/status print between compute() and advanceTime.  After isph_ins_solve. */
int isph_ins_diagnostics(isph_ins *S, double t, double out[12] /*host*/);
/* nsteps times: isph_ins_rebuild (when the particles have moved since the list was taken, or there is none), pre, solve,
 * diagnostics, advance, shift when shift > 0.  diag: host [nsteps][16] or NULL; a row is isph_ins_diagnostics at
 * t = step dt (steps count from 1 over the life of the state), then the Helmholtz and Poisson iteration counts and their
 * converged flags. */
int isph_ins_run(isph_ins *S, int nsteps, double *diag);

/* ---- the same driver on a brick of ranks ---------------------------------------------------------------------------- */

/* An isph_ins made by isph_ins_create_dist owns ONE RANK's share of the particles and runs the same phases COLLECTIVELY
 * over the decomposition: every rank makes every call.  The context has RCCL, the host-staged transport, or no
 * communicator (a 1 x 1 (x 1) grid; the results then equal the one-rank driver's bit for bit).  The decomposition is
 * copied, faces included.  Refused by name: prm->cut <= 0; a grid whose product differs from the context's rank count; a
 * sub-box narrower than the cut; prm->lo / hi / periodic that are set (not all zero) and differ from the decomposition's;
 * and what isph_ins_create refuses (block Helmholtz, MorrisHolmes, bd_coord / use_part, recycle, hold-pattern mode).
 *
 * isph_ins_set_state_dist: the particles this rank holds (nlocal = 0 allowed) with `tag`, the caller's global id, an int
 * carried with the particle.  They must lie in the rank's sub-box or in a grid neighbour's: the first rebuild migrates
 * them.  ONE sum all-reduce: the non-Solid rows of all ranks (the value of the SA-AMG null vector), the Solid rows, the
 * particles, the failure flag -- a type outside [1, ntypes] on one rank fails ALL ranks, the others with "... failed on
 * another rank".  isph_ins_set_state and isph_ins_set_list are refused on such a state by name.
 *
 * isph_ins_rebuild on such a state: v, p, rho, nu -> [nlocal][6] doubles, type, tag -> [nlocal][2] ints (one kernel);
 * isph_migrate; unpack (one kernel); isph_nlist_build_dist with prune = 1; ONE isph_nlist_forward_multi of v, p, rho, nu,
 * type, tag; the host null mask of isph_solve is remade from the types (a read-back of nlocal ints) only when a particle
 * arrived or left.  Every other phase is the one-rank phase with: the forward through the list's plan for the ghost
 * fills; the list's colmap and ncol, rank0 = (rank == 0) in the assemblers; isph_mat_set_halo from the list's plan on H
 * and A; owned rows of vstar then its forward; the *_dist forms of the zero mean, the TGV error and the status; normals
 * and pnd in ONE forward of 4 doubles per ghost.  A rank that fails in a phase carries its rc to the next consensus
 * (before migration, before the list build, before the forward of the state, after each assembly), where all fail.
 * isph_ins_get knows "tag", "owner_rank" and "colmap" on such a state; "owner" is the index on the owner's rank.
 * The diag rows of isph_ins_run are the same bits on every rank. */
int isph_ins_create_dist(isph_ctx *ctx, const isph_ins_params *prm, const isph_decomp *dc, isph_ins **S);
int isph_ins_set_state_dist(isph_ins *S, int nlocal, const double *x, const double *v, const double *p, const int *type,
                            const double *rho, const double *nu, const int *tag, int on_device);
/* info: [0] nlocal [1] nall [2] list entries (-1: no list) [3] steps [4] ncol [5] npeers [6] off-rank ghosts
 * [7] particles sent and [8] received by the last rebuild [9] the particle count over all ranks */
int isph_ins_sizes_dist(const isph_ins *S, long long info[10]);

#ifdef __cplusplus
}
#endif
#endif
