// pattern.hpp -- the entry map of a matrix whose pattern is kept (isph_ctx_hold_pattern).
//
// Within one time step the reference refills ONE Epetra matrix -- one graph -- with new values several times
// (pair_isph.cpp:1266-1270 allocates A.crs, :589 :636 :812 :925 :988-1011 refill and solve it; Epetra's
// ReplaceMyValues keeps the graph).  The map is what makes the same possible here: emap[e] = position in S.val (and
// S.col) of entry e of the CSR the matrix was created from, in the caller's entry order, through everything the ingress
// did to the entry -- the row sort of unsorted rows, and on the routes with coordinates the library's row permutation,
// the renaming of the owned columns and the sort by the new column.  isph_mat_update_values is then one scatter
// sval[emap[e]] = val[e]: no arithmetic, so the updated matrix is bit for bit the matrix a fresh create gives.
//
// The map is built on the device from what the conversion leaves there: one lane per row of the source image (the
// caller's device CSR, or the chunked image of the host ingress -- sell.hpp CsrChunks -- which is still resident when
// the conversion has finished) walks its source columns front to back, exactly like k_csr_to_sell, and searches each one
// in its finished, column-sorted sliced-ELL row.  The route that permutes AFTER the ingress (isph_mat_create_csr_coords)
// sends the finished map through the permutation with one thread per entry (k_pattern_remap).
// An entry of the map is a 32-bit position: 4 B per entry of the CSR (a 16-bit in-row slot would need the row of an entry
// besides, i.e. a search of the row pointers per scattered value); a matrix with 2^32 or more stored positions gets none.
// A row that holds a column twice cannot be mapped by a search (Epetra never hands one over after FillComplete): the
// kernel raises a flag and the matrix is created as without the mode, without a map.
#pragma once
#include "core.hpp"
#include "sell.hpp"

namespace isph {

// position of column c in the sorted row (off, lane, len), -1 when the row does not hold it
__device__ __forceinline__ long long pattern_find(const int *__restrict__ scol, long long off, int lane, int len, int c) {
  int lo = 0, hi = len - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (scol[sell_pos(off, lane, mid)] < c) lo = mid + 1; else hi = mid;
  }
  const long long p = sell_pos(off, lane, lo);
  return (len > 0 && scol[p] == c) ? p : -1;
}

// Source image: rowptr + colidx (device CSR, ck.stage == nullptr) or rowptr + the chunked image ck, read like
// k_csr_to_sell reads it.  Row r of the image is row r of the matrix; ebase (may be NULL: rowptr) gives the first entry of
// the row in the CALLER's entry order -- they differ when the staging threads gathered the rows in the library's order
// (ingress.hpp IngressGather), whose columns colren renames.  flag: 1 a row holds a column twice, 2 a column was not found.
template <class OFF>
__global__ void k_pattern_map(int nrow, const OFF *__restrict__ rowptr, const int *__restrict__ colidx, CsrChunks ck,
                              const int *__restrict__ colren, int nren, const int *__restrict__ ebase,
                              const long long *__restrict__ slice_off, const int *__restrict__ scol,
                              unsigned *__restrict__ emap, int *__restrict__ flag) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= nrow) return;
  const OFF beg = rowptr[row];
  const int len = (int)(rowptr[row + 1] - beg);
  if (len == 0) return;
  const long long off = slice_off[row >> 6];
  const int lane = row & 63;
  {
    int pc = scol[sell_pos(off, lane, 0)];
    bool dup = false;
    for (int k = 1; k < len; ++k) {
      const int c = scol[sell_pos(off, lane, k)];
      dup = dup || c == pc;
      pc = c;
    }
    if (dup) { atomicOr(flag, 1); return; }
  }
  const bool chunked = ck.stage != nullptr;
  int ch = 0;
  ChunkView cv{};
  int first_col = 0;
  if (chunked) {  // chunk of the row's first entry
    int lo = 0, hi = ck.nchunks - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (ck.cstart[mid] <= (long long)beg) lo = mid; else hi = mid - 1;
    }
    ch = lo;
    cv = chunk_view(ck, ch);
    first_col = cv.m16 ? cv.rowfirst[row - cv.row0] : cv.c32[(long long)beg - cv.cbase];
  }
  const long long eb = ebase ? (long long)ebase[row] : (long long)beg;
  int prev = 0;
  for (int k = 0; k < len; ++k) {
    const long long q = (long long)beg + k;
    int c;
    if (!chunked) {
      c = colidx[q];
    } else {
      if (q >= cv.cend) cv = chunk_view(ck, ++ch);
      const long long e = q - cv.cbase;
      if (!cv.m16) c = cv.c32[e];
      else if (k == 0) c = first_col;
      else c = prev + (int)cv.d16[e];
    }
    prev = c;
    if (colren && c < nren) c = colren[c];
    const long long p = pattern_find(scol, off, lane, len, c);
    if (p < 0) atomicOr(flag, 2);
    else emap[eb + k] = (unsigned)p;
  }
}

// the map of matrix 0 through a symmetric permutation (sell_permute: row i of matrix 0 is row iperm[i] of the result,
// owned columns renamed through iperm, rows sorted by the new column); one thread per entry, in place
__global__ void k_pattern_remap(long long nnz, int nrow, int nslices0, const long long *__restrict__ slice_off0,
                                const int *__restrict__ scol0, const int *__restrict__ iperm,
                                const int *__restrict__ rowlen, const long long *__restrict__ slice_off,
                                const int *__restrict__ scol, unsigned *__restrict__ emap, int *__restrict__ flag) {
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < nnz; e += (long long)gridDim.x * blockDim.x) {
    const long long p0 = (long long)emap[e];
    int lo = 0, hi = nslices0 - 1;  // slice of position p0
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (slice_off0[mid] <= p0) lo = mid; else hi = mid - 1;
    }
    const int row0 = lo * kSlice + (int)(((p0 - slice_off0[lo]) & 127) >> 1);
    int c = scol0[p0];
    if (c < nrow) c = iperm[c];
    const int r = iperm[row0];
    const long long p = pattern_find(scol, slice_off[r >> 6], r & 63, rowlen[r], c);
    if (p < 0) atomicOr(flag, 2);
    else emap[e] = (unsigned)p;
  }
}

// sval[emap[e]] = v[e - e0] for the entries [e0, e0 + n) of the caller's CSR
__global__ void k_pattern_scatter(long long e0, long long n, const double *__restrict__ v, const unsigned *__restrict__ emap,
                                  double *__restrict__ sval) {
  for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (long long)gridDim.x * blockDim.x)
    sval[emap[e0 + k]] = __builtin_nontemporal_load(&v[k]);
}

inline int pattern_grid(long long n) { return (int)std::min<long long>((n + kBlock - 1) / kBlock, 8192); }

// true when a matrix of this shape can carry a map at all (32-bit positions)
inline bool pattern_mappable(const Sell &S) { return S.nnz > 0 && S.stored < (1LL << 32); }

// reads the flag behind everything queued; a matrix whose flag is raised loses its map (created as without the mode)
inline int pattern_finish(isph_ctx *ctx, isph_mat *A, const int *flag_dev) {
  int flag = 0;
  ISPH_CHECK_HIP(hipMemcpyAsync(&flag, flag_dev, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  ISPH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  ISPH_CHECK_HIP(hipGetLastError());
  if (flag & 1) { A->emap.release(); return ISPH_SUCCESS; }  // a column twice in a row
  ISPH_REQUIRE(flag == 0, "entry map: a source column was not found in its sliced-ELL row");
  return ISPH_SUCCESS;
}

// the map of a finished matrix from its source image (see k_pattern_map); host-synchronous
template <class OFF>
inline int pattern_build(isph_ctx *ctx, isph_mat *A, const OFF *drowptr, const int *dcolidx, const CsrChunks &ck,
                         const int *colren, int nren, const int *debase) {
  const Sell &S = A->S;
  if (!pattern_mappable(S)) return ISPH_SUCCESS;
  DevTmp<int> flag;
  ISPH_CHECK(flag.reserve(1));
  ISPH_CHECK(A->emap.reserve((size_t)S.nnz));
  ISPH_CHECK_HIP(hipMemsetAsync(flag.p, 0, sizeof(int), ctx->stream));
  hipLaunchKernelGGL(k_pattern_map<OFF>, dim3((S.nrow + kBlock - 1) / kBlock), dim3(kBlock), 0, ctx->stream, S.nrow, drowptr, dcolidx, ck,
                     colren, nren, debase, (const long long *)S.slice_off.p, (const int *)S.col.p, A->emap.p, flag.p);
  return pattern_finish(ctx, A, flag.p);
}

// A0 (with its map) was permuted into A (sell_permute with the order O): the map moves to A
inline int pattern_remap(isph_ctx *ctx, isph_mat *A0, const int *iperm, isph_mat *A) {
  if (!A0->emap.p) return ISPH_SUCCESS;
  const Sell &S0 = A0->S, &S = A->S;
  DevTmp<int> flag;
  ISPH_CHECK(flag.reserve(1));
  ISPH_CHECK_HIP(hipMemsetAsync(flag.p, 0, sizeof(int), ctx->stream));
  hipLaunchKernelGGL(k_pattern_remap, dim3(pattern_grid(S.nnz)), dim3(kBlock), 0, ctx->stream, S.nnz, S.nrow, S0.nslices,
                     (const long long *)S0.slice_off.p, (const int *)S0.col.p, iperm, (const int *)S.rowlen.p,
                     (const long long *)S.slice_off.p, (const int *)S.col.p, A0->emap.p, flag.p);
  A->emap = A0->emap;
  A0->emap = DevBuf<unsigned>();
  return pattern_finish(ctx, A, flag.p);
}

}  // namespace isph
