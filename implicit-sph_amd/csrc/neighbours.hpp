// neighbours.hpp -- ghost atoms and the full neighbour list of one rank, built on the device (isph_nlist_*).
//
// The device twin of isph_cloud_build (workload.cpp): wrap the owned particles into the box, create the periodic images
// within the cut of a face, and list for every owned particle the particles closer than the cut, in ascending particle
// index.  For a fully periodic box with lo = 0 the result equals the host's bit for bit, which needs three things:
//   * the wrap is fmod + the two fix-ups of numpy's mod (exact on both sides);
//   * the images are placed by a count per owner, an exclusive scan and a fill -- no atomics whose arrival order shows;
//   * the distance is ((d0 d0) + d1 d1) + d2 d2 with every product and sum rounded: the host library is built without an
//     FMA target, so the device functions below switch contraction off (a fused rsq decides pairs that lie on the cut
//     radius of a lattice differently).
//
// Stages (all queued on the context's stream; the host reads back the number of ghosts and the number of list entries,
// nothing else -- the cell grid is sized on the device from the bounding box of owned + ghost particles):
//   1 k_nl_wrap_count   wrapped owned positions, images per owner              -> exclusive scan -> nghost
//   2 k_nl_images       x_all = owned + images, owner_index
//   3 k_order_bbox + k_nl_grid   cells of edge >= cut over the particles' extent (device-resident geometry)
//   4 k_nl_cell_keys + stable radix sort by cell + k_nl_gather   the cell-sorted copy: positions as three coordinate
//     arrays and the original index; inside a cell the original indices ascend; for fixed (cy, cz) the x-adjacent cells
//     are one contiguous run, so a home cell reads 9 runs in 3-D and 3 in 2-D
//   5 k_nl_search<COUNT> -> exclusive scan of the row lengths (64-bit) -> nnz -> k_nl_search<FILL>
//     one wave per owned particle, 64 candidates per step read from the cell-sorted arrays, ballot + prefix-count
//     compaction.  Rows of up to kNlLdsRow entries are collected in LDS, rank-sorted there by original index and written
//     out coalesced; longer rows (a dense clump) are written unsorted and sorted in place by their wave with a bitonic
//     network in global memory.  Candidates always come from global memory (L2): no staging that a dense cell could
//     overflow.
// Stages 3 - 5 are nl_list_rows, which the multi-rank build (nlist_dist.hpp) runs over its own owned + ghost particles.
#pragma once
#include <rocprim/rocprim.hpp>

#include <climits>

#include "common.hpp"
#include "core.hpp"
#include "order.hpp"

struct isph_nlist {
  int dim = 0, nlocal = 0, nghost = 0, fits32 = 0;
  long long nnz = 0;
  isph::DevBuf<double> x;          // [nall][3]
  isph::DevBuf<int> owner;         // [nall]
  isph::DevBuf<long long> ptr64;   // [nlocal + 1]
  isph::DevBuf<int> ptr32;         // [nlocal + 1] when fits32
  isph::DevBuf<int> idx;           // [nnz]
  // a list built across ranks (nlist_dist.hpp): owner rank and matrix column of every particle, the halo plan
  int dist = 0, ncol = 0, noffrank = 0;
  isph::DevBuf<int> orank, colmap;  // [nall]
  isph_halo halo;                   // peers, send / receive ranges, send_idx: the plan of isph_nlist_forward
  void release() {
    x.release(); owner.release(); ptr64.release(); ptr32.release(); idx.release();
    orank.release(); colmap.release(); halo.send_idx.release();
  }
};

namespace isph {

constexpr int kNlLdsRow = 1024;     // longest row that is sorted in LDS
constexpr int kNlMaxCells = 1 << 24;

struct NlBox {
  int dim, wrap;
  double lo[3], hi[3], period[3], cut;
  int periodic[3];
};

struct NlGrid {      // lives in device memory: written by k_nl_grid, read by the kernels after it
  double org[3], inv[3];
  int nc[3];
};

__device__ inline double nl_wrap(double x, double lo, double period) {
  double r = fmod(x - lo, period);
  if (r < 0.0) r += period;
  if (r >= period) r = 0.0;
  return r + lo;
}

// image shifts of a (wrapped) particle: lo_s[a] .. hi_s[a] on every axis
__device__ inline int nl_shifts(const NlBox &b, const double *p, int *lo_s, int *hi_s) {
  int cnt = 1;
  for (int a = 0; a < 3; ++a) {
    lo_s[a] = hi_s[a] = 0;
    if (a >= b.dim || !b.periodic[a]) continue;
    if (p[a] - b.lo[a] < b.cut) hi_s[a] = 1;
    if (p[a] >= b.hi[a] - b.cut) lo_s[a] = -1;
    cnt *= 1 + hi_s[a] - lo_s[a];
  }
  return cnt - 1;
}

__global__ void k_nl_wrap_count(int n, NlBox b, const double *__restrict__ x, double *__restrict__ xw, int *__restrict__ cnt) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double p[3];
  for (int a = 0; a < 3; ++a) {
    p[a] = x[3 * (size_t)i + a];
    if (b.wrap && a < b.dim && b.periodic[a]) p[a] = nl_wrap(p[a], b.lo[a], b.period[a]);
    xw[3 * (size_t)i + a] = p[a];
  }
  int lo_s[3], hi_s[3];
  cnt[i] = nl_shifts(b, p, lo_s, hi_s);
}

// goff: exclusive scan of the image counts.  Image order of an owner: sz, sy, sx from the outer to the inner loop.
__global__ void k_nl_images(int n, NlBox b, const double *__restrict__ xw, const int *__restrict__ goff, double *__restrict__ xall,
                            int *__restrict__ owner) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double p[3];
  for (int a = 0; a < 3; ++a) {
    p[a] = xw[3 * (size_t)i + a];
    xall[3 * (size_t)i + a] = p[a];
  }
  owner[i] = i;
  int lo_s[3], hi_s[3];
  if (nl_shifts(b, p, lo_s, hi_s) == 0) return;
  size_t g = (size_t)n + (size_t)goff[i];
  for (int sz = lo_s[2]; sz <= hi_s[2]; ++sz)
    for (int sy = lo_s[1]; sy <= hi_s[1]; ++sy)
      for (int sx = lo_s[0]; sx <= hi_s[0]; ++sx) {
        if (!sx && !sy && !sz) continue;
        // s is -1, 0 or 1: the product is exact, so the sum is rounded once whether or not it is fused
        xall[3 * g] = p[0] + (double)sx * b.period[0];
        xall[3 * g + 1] = p[1] + (double)sy * b.period[1];
        xall[3 * g + 2] = b.dim == 3 ? p[2] + (double)sz * b.period[2] : 0.0;
        owner[g] = i;
        ++g;
      }
}

// Cell grid from the per-workgroup bounding boxes of k_order_bbox: floor(extent / cut) cells per axis with a margin of
// 1e-6 on the edge (so that the rounding of the cell index, about 2^-32 of a cell at 2^20 cells, never puts two
// particles closer than the cut into cells that are not adjacent), halved along the longest axis until no more than
// `cap` cells remain.  One thread.
__global__ __launch_bounds__(kWave) void k_nl_grid(int nparts, const double *__restrict__ part, int dim, double cut, int cap, NlGrid *__restrict__ g) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  double mn[3] = {1e300, 1e300, 1e300}, mx[3] = {-1e300, -1e300, -1e300};
  for (int k = 0; k < nparts; ++k)
    for (int a = 0; a < 3; ++a) {
      mn[a] = fmin(mn[a], part[(size_t)k * 6 + a]);
      mx[a] = fmax(mx[a], part[(size_t)k * 6 + 3 + a]);
    }
  int nc[3] = {1, 1, 1};
  double ext[3] = {0.0, 0.0, 0.0};
  for (int a = 0; a < dim; ++a) {
    ext[a] = mx[a] - mn[a];
    const double q = floor(ext[a] / (cut * 1.000001));
    nc[a] = !(q >= 1.0) ? 1 : (q > 1048576.0 ? 1048576 : (int)q);
  }
  while ((long long)nc[0] * nc[1] * nc[2] > (long long)cap) {
    int a = 0;
    if (nc[1] > nc[a]) a = 1;
    if (nc[2] > nc[a]) a = 2;
    nc[a] = (nc[a] + 1) / 2;
  }
  for (int a = 0; a < 3; ++a) {
    g->nc[a] = nc[a];
    g->org[a] = nc[a] > 1 ? mn[a] : 0.0;
    g->inv[a] = nc[a] > 1 ? (double)nc[a] / ext[a] : 0.0;
  }
}

__device__ inline int nl_cell(const NlGrid &g, int a, double x) {
  const int n = g.nc[a];
  if (n <= 1) return 0;
  const double t = floor((x - g.org[a]) * g.inv[a]);
  return !(t >= 1.0) ? 0 : (t >= (double)n ? n - 1 : (int)t);
}

__global__ void k_nl_cell_keys(int nall, const NlGrid *__restrict__ gp, const double *__restrict__ x, unsigned *__restrict__ key,
                               int *__restrict__ val, int *__restrict__ hist) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nall) return;
  const NlGrid g = *gp;
  const int c0 = nl_cell(g, 0, x[3 * (size_t)j]), c1 = nl_cell(g, 1, x[3 * (size_t)j + 1]), c2 = nl_cell(g, 2, x[3 * (size_t)j + 2]);
  const unsigned c = ((unsigned)c2 * (unsigned)g.nc[1] + (unsigned)c1) * (unsigned)g.nc[0] + (unsigned)c0;
  key[j] = c;
  val[j] = j;
  atomicAdd(&hist[c], 1);   // a count: the order of arrival does not show
}

__global__ void k_nl_gather(int nall, const int *__restrict__ order, const double *__restrict__ x, double *__restrict__ s0,
                            double *__restrict__ s1, double *__restrict__ s2) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nall) return;
  const size_t j = (size_t)order[q];
  s0[q] = x[3 * j];
  s1[q] = x[3 * j + 1];
  s2[q] = x[3 * j + 2];
}

struct NlSorted {
  int nall, nlocal, dim;
  double cutsq;
  const NlGrid *grid;
  const int *cstart;       // [cells + 1]
  const unsigned *ckey;    // [nall] cell of the sorted slot
  const int *sid;          // [nall] original index of the sorted slot, ascending inside a cell
  const double *s0, *s1, *s2;
};

// squared distance exactly as the host computes it: every product and every sum rounded
__device__ inline double nl_rsq(double d0, double d1, double d2) {
#pragma clang fp contract(off)
  double r = d0 * d0;
  r = r + d1 * d1;
  r = r + d2 * d2;
  return r;
}

// in-place ascending sort of row[0 .. n) by one wave: the bitonic network whose merges start with a flip (t ^ (k - 1)), so
// that every compare-exchange puts the smaller value at the lower index and partners past the end (virtual +infinity)
// are simply skipped -- any n, no padding.  The passes are separated by a device-scope fence: a lane reads what other
// lanes of its wave wrote in the pass before.
__device__ inline void nl_sort_global(int *rowp, long long n, int lane) {
  volatile int *row = rowp;
  for (long long k = 2; (k >> 1) < n; k <<= 1) {
    for (long long j = k; j > 1; j >>= 1) {
      const long long mask = (j == k) ? k - 1 : (j >> 1);
      for (long long t = lane; t < n; t += kWave) {
        const long long l = t ^ mask;
        if (l > t && l < n) {
          const int a = row[t], b = row[l];
          if (a > b) { row[t] = b; row[l] = a; }
        }
      }
      __threadfence();
    }
  }
}

// One wave (= one workgroup) per cell-sorted slot; slots of ghosts leave at once.  FILL = 0: cnt[i] = row length.
// FILL = 1: the row of i, ascending, at idx[ptr[i] ..).
template <int FILL>
__global__ __launch_bounds__(kWave) void k_nl_search(NlSorted S, long long *__restrict__ cnt, const long long *__restrict__ ptr,
                                                     int *__restrict__ idx) {
  __shared__ __attribute__((aligned(16))) int buf_a[FILL ? kNlLdsRow : 4];
  __shared__ int buf_b[FILL ? kNlLdsRow : 4];
  const int q = blockIdx.x, lane = threadIdx.x;
  const int i = S.sid[q];
  if (i >= S.nlocal) return;
  const NlGrid g = *S.grid;
  const double x0 = S.s0[q], x1 = S.s1[q], x2 = S.s2[q];
  unsigned c = S.ckey[q];
  const int cx = (int)(c % (unsigned)g.nc[0]);
  c /= (unsigned)g.nc[0];
  const int cy = (int)(c % (unsigned)g.nc[1]), cz = (int)(c / (unsigned)g.nc[1]);
  const int xl = cx > 0 ? cx - 1 : 0, xh = cx + 1 < g.nc[0] ? cx + 1 : g.nc[0] - 1;
  long long base = 0, len = 0;
  if (FILL) { base = ptr[i]; len = ptr[i + 1] - base; }
  const bool in_lds = FILL && len <= kNlLdsRow;
  long long n = 0;
  for (int oz = -1; oz <= 1; ++oz) {
    const int z = cz + oz;
    if (z < 0 || z >= g.nc[2]) continue;
    for (int oy = -1; oy <= 1; ++oy) {
      const int y = cy + oy;
      if (y < 0 || y >= g.nc[1]) continue;
      const size_t rowc = ((size_t)z * g.nc[1] + y) * g.nc[0];
      const int begin = S.cstart[rowc + xl], end = S.cstart[rowc + xh + 1];
      for (int k0 = begin; k0 < end; k0 += kWave) {
        const int k = k0 + lane;
        bool hit = false;
        int j = 0;
        if (k < end) {
          j = S.sid[k];
          const double d0 = x0 - S.s0[k], d1 = x1 - S.s1[k], d2 = S.dim == 3 ? x2 - S.s2[k] : 0.0;
          hit = j != i && nl_rsq(d0, d1, d2) < S.cutsq;
        }
        const unsigned long long m = __ballot(hit);
        if (FILL) {
          const long long pos = n + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
          if (hit && pos < len) {     // pos < len always (the count pass ran the same tests); the guard keeps a store in bounds
            if (in_lds) buf_a[pos] = j; else idx[base + pos] = j;
          }
        }
        n += __popcll(m);
      }
    }
  }
  if (!FILL) {
    if (lane == 0) cnt[i] = n;
    return;
  }
  if (!in_lds) {
    __threadfence();
    nl_sort_global(idx + base, len, lane);
    return;
  }
  // rank sort in LDS: the entries of a row are distinct particle indices, so rank = number of smaller entries
  const int nr = (int)len, n4 = (nr + 3) & ~3;
  if (lane < n4 - nr) buf_a[nr + lane] = INT_MAX;
  __syncthreads();
  for (int t = lane; t < nr; t += kWave) {
    const int e = buf_a[t];
    int r = 0;
    for (int k = 0; k < n4; k += 4) {
      const int4 v = *reinterpret_cast<const int4 *>(&buf_a[k]);
      r += (v.x < e) + (v.y < e) + (v.z < e) + (v.w < e);
    }
    buf_b[r] = e;
  }
  __syncthreads();
  for (int t = lane; t < nr; t += kWave) idx[base + t] = buf_b[t];
}

__global__ void k_nl_ptr32(int n1, const long long *__restrict__ p64, int *__restrict__ p32) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n1) p32[i] = (int)p64[i];
}

template <class T>
inline int nl_exclusive_scan(hipStream_t st, const T *in, T *out, size_t n) {
  size_t bytes = 0;
  ISPH_CHECK_HIP(rocprim::exclusive_scan(nullptr, bytes, in, out, T(0), n, rocprim::plus<T>(), st));
  DevTmp<char> tmp;
  ISPH_CHECK(tmp.reserve(bytes > 0 ? bytes : 1));
  ISPH_CHECK_HIP(rocprim::exclusive_scan(tmp.p, bytes, in, out, T(0), n, rocprim::plus<T>(), st));
  return ISPH_SUCCESS;
}

inline int nl_check_box(int dim, int nlocal, const double lo[3], const double hi[3], const int periodic[3], double cut) {
  ISPH_REQUIRE(dim == 2 || dim == 3, "dim must be 2 or 3");
  ISPH_REQUIRE(nlocal >= 0 && nlocal <= INT_MAX / 8, "nlocal out of range");
  ISPH_REQUIRE(cut > 0.0, "cut must be positive");
  for (int a = 0; a < dim; ++a)
    if (periodic[a]) ISPH_REQUIRE(hi[a] - lo[a] >= 2.0 * cut, "a periodic axis is shorter than two cuts");
  return ISPH_SUCCESS;
}

// Stages 3 - 5: the rows of the n owned particles over the nall particles of L.x (owned first), into L.ptr64 / ptr32 / idx.
inline int nl_list_rows(isph_ctx *ctx, int dim, int n, int nall, double cut, isph_nlist &L) {
  hipStream_t st = ctx->stream;
  const dim3 blk(kBlock);
  // 3. the cell grid, on the device
  const dim3 grid_all((nall + kBlock - 1) / kBlock);
  const int gb = std::min(256, (nall + kBlock - 1) / kBlock);
  const int cap = std::max(1, std::min(nall, kNlMaxCells));
  DevTmp<double> part;
  DevTmp<NlGrid> dgrid;
  ISPH_CHECK(part.reserve((size_t)gb * 6));
  ISPH_CHECK(dgrid.reserve(1));
  OrderGeom og;
  memset(&og, 0, sizeof(og));
  og.dim = dim;
  hipLaunchKernelGGL(k_order_bbox, dim3(gb), blk, 0, st, nall, og, (const double *)L.x.p, part.p);
  hipLaunchKernelGGL(k_nl_grid, dim3(1), dim3(64), 0, st, gb, (const double *)part.p, dim, cut, cap, dgrid.p);
  // 4. the cell-sorted copy
  DevTmp<unsigned> key0, key1;
  DevTmp<int> val0, sid, hist, cstart;
  DevTmp<double> s0, s1, s2;
  DevTmp<char> tmp;
  ISPH_CHECK(key0.reserve((size_t)nall));
  ISPH_CHECK(key1.reserve((size_t)nall));
  ISPH_CHECK(val0.reserve((size_t)nall));
  ISPH_CHECK(sid.reserve((size_t)nall));
  ISPH_CHECK(hist.reserve((size_t)cap + 1));
  ISPH_CHECK(cstart.reserve((size_t)cap + 1));
  ISPH_CHECK(s0.reserve((size_t)nall));
  ISPH_CHECK(s1.reserve((size_t)nall));
  ISPH_CHECK(s2.reserve((size_t)nall));
  ISPH_CHECK_HIP(hipMemsetAsync(hist.p, 0, sizeof(int) * ((size_t)cap + 1), st));
  hipLaunchKernelGGL(k_nl_cell_keys, grid_all, blk, 0, st, nall, (const NlGrid *)dgrid.p, (const double *)L.x.p, key0.p, val0.p, hist.p);
  ISPH_CHECK(nl_exclusive_scan<int>(st, hist.p, cstart.p, (size_t)cap + 1));
  unsigned bits = 1;
  while (bits < 32 && (((unsigned)cap - 1u) >> bits) != 0) ++bits;
  size_t bytes = 0;
  ISPH_CHECK_HIP(rocprim::radix_sort_pairs(nullptr, bytes, key0.p, key1.p, val0.p, sid.p, (size_t)nall, 0u, bits, st));
  ISPH_CHECK(tmp.reserve(bytes > 0 ? bytes : 1));
  ISPH_CHECK_HIP(rocprim::radix_sort_pairs(tmp.p, bytes, key0.p, key1.p, val0.p, sid.p, (size_t)nall, 0u, bits, st));
  hipLaunchKernelGGL(k_nl_gather, grid_all, blk, 0, st, nall, (const int *)sid.p, (const double *)L.x.p, s0.p, s1.p, s2.p);
  key0.release(); val0.release(); hist.release(); tmp.release(); part.release();
  // 5. count, offsets, fill
  NlSorted S;
  S.nall = nall; S.nlocal = n; S.dim = dim; S.cutsq = cut * cut;
  S.grid = dgrid.p; S.cstart = cstart.p; S.ckey = key1.p; S.sid = sid.p;
  S.s0 = s0.p; S.s1 = s1.p; S.s2 = s2.p;
  DevTmp<long long> cnt;
  ISPH_CHECK(cnt.reserve((size_t)n + 1));
  ISPH_CHECK_HIP(hipMemsetAsync(cnt.p + n, 0, sizeof(long long), st));
  hipLaunchKernelGGL(k_nl_search<0>, dim3(nall), dim3(kWave), 0, st, S, cnt.p, (const long long *)nullptr, (int *)nullptr);
  ISPH_CHECK(nl_exclusive_scan<long long>(st, cnt.p, L.ptr64.p, (size_t)n + 1));
  long long nnz = 0;
  ISPH_CHECK_HIP(hipMemcpyAsync(&nnz, L.ptr64.p + n, sizeof(long long), hipMemcpyDeviceToHost, st));
  ISPH_CHECK_HIP(hipStreamSynchronize(st));
  ISPH_CHECK_HIP(hipGetLastError());
  ISPH_REQUIRE(nnz >= 0, "neighbour count failed");
  cnt.release();
  L.nnz = nnz;
  L.fits32 = nnz < (long long)INT_MAX ? 1 : 0;   // the rule of workload.py: fewer than 2^31 - 1 entries
  ISPH_CHECK(L.idx.reserve((size_t)(nnz > 0 ? nnz : 1)));
  if (nnz > 0)
    hipLaunchKernelGGL(k_nl_search<1>, dim3(nall), dim3(kWave), 0, st, S, (long long *)nullptr, (const long long *)L.ptr64.p, L.idx.p);
  if (L.fits32) {
    ISPH_CHECK(L.ptr32.reserve((size_t)n + 1));
    hipLaunchKernelGGL(k_nl_ptr32, dim3((n + 1 + kBlock - 1) / kBlock), blk, 0, st, n + 1, (const long long *)L.ptr64.p, L.ptr32.p);
  }
  ISPH_CHECK_HIP(hipStreamSynchronize(st));
  ISPH_CHECK_HIP(hipGetLastError());
  return ISPH_SUCCESS;
}

inline int nlist_build(isph_ctx *ctx, int dim, int nlocal, const double *x, const double lo[3], const double hi[3],
                       const int periodic[3], double cut, int wrap, int on_device, isph_nlist &L) {
  hipStream_t st = ctx->stream;
  NlBox b;
  memset(&b, 0, sizeof(b));
  b.dim = dim; b.wrap = wrap != 0; b.cut = cut;
  for (int a = 0; a < 3; ++a) {
    b.lo[a] = lo[a]; b.hi[a] = hi[a]; b.period[a] = hi[a] - lo[a];
    b.periodic[a] = a < dim && periodic[a] != 0;
  }
  const int n = nlocal;
  L.dim = dim; L.nlocal = n;
  ISPH_CHECK(L.ptr64.reserve((size_t)n + 1));
  if (n == 0) {
    ISPH_CHECK_HIP(hipMemsetAsync(L.ptr64.p, 0, sizeof(long long), st));
    ISPH_CHECK(L.ptr32.reserve(1));
    ISPH_CHECK_HIP(hipMemsetAsync(L.ptr32.p, 0, sizeof(int), st));
    ISPH_CHECK_HIP(hipStreamSynchronize(st));
    L.fits32 = 1;
    return ISPH_SUCCESS;
  }
  const dim3 blk(kBlock), grid_n((n + kBlock - 1) / kBlock);
  // 1. wrap, images per owner, their offsets
  DevTmp<double> xin, xw;
  const double *dx = x;
  if (!on_device) {
    ISPH_REQUIRE(!is_device_pointer(x), "on_device = 0 but x is device memory");
    ISPH_CHECK(xin.reserve((size_t)n * 3));
    ISPH_CHECK_HIP(hipMemcpyAsync(xin.p, x, sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice, st));
    dx = xin.p;
  }
  DevTmp<int> gcnt, goff;
  ISPH_CHECK(xw.reserve((size_t)n * 3));
  ISPH_CHECK(gcnt.reserve((size_t)n + 1));
  ISPH_CHECK(goff.reserve((size_t)n + 1));
  ISPH_CHECK_HIP(hipMemsetAsync(gcnt.p + n, 0, sizeof(int), st));
  hipLaunchKernelGGL(k_nl_wrap_count, grid_n, blk, 0, st, n, b, dx, xw.p, gcnt.p);
  ISPH_CHECK(nl_exclusive_scan<int>(st, gcnt.p, goff.p, (size_t)n + 1));
  int nghost = 0;
  ISPH_CHECK_HIP(hipMemcpyAsync(&nghost, goff.p + n, sizeof(int), hipMemcpyDeviceToHost, st));
  ISPH_CHECK_HIP(hipStreamSynchronize(st));
  ISPH_REQUIRE(nghost >= 0 && (long long)n + nghost < INT_MAX, "too many particles");
  const int nall = n + nghost;
  L.nghost = nghost;
  // 2. owned + images
  ISPH_CHECK(L.x.reserve((size_t)nall * 3));
  ISPH_CHECK(L.owner.reserve((size_t)nall));
  hipLaunchKernelGGL(k_nl_images, grid_n, blk, 0, st, n, b, (const double *)xw.p, (const int *)goff.p, L.x.p, L.owner.p);
  xin.release(); xw.release(); gcnt.release(); goff.release();
  return nl_list_rows(ctx, dim, n, nall, cut, L);
}

template <class T>
inline int nl_copy_out(isph_ctx *ctx, T *dst, const T *src, size_t count, int on_device) {
  if (!dst || count == 0) return ISPH_SUCCESS;
  ISPH_REQUIRE(on_device || !is_device_pointer(dst), "on_device = 0 but an output is device memory");
  ISPH_CHECK_HIP(hipMemcpyAsync(dst, src, sizeof(T) * count, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
  return ISPH_SUCCESS;
}

}  // namespace isph

extern "C" {

int isph_nlist_build(isph_ctx *ctx, int dim, int nlocal, const double *x, const double lo[3], const double hi[3],
                     const int periodic[3], double cut, int wrap, int on_device, isph_nlist **out) {
  using namespace isph;
  ISPH_REQUIRE(ctx && lo && hi && periodic && out, "NULL argument");
  ISPH_CHECK(nl_check_box(dim, nlocal, lo, hi, periodic, cut));
  ISPH_REQUIRE(x || nlocal == 0, "x is NULL");
  isph_nlist *L = new isph_nlist();
  const int rc = nlist_build(ctx, dim, nlocal, x, lo, hi, periodic, cut, wrap, on_device, *L);
  if (rc != ISPH_SUCCESS) {
    L->release();
    delete L;
    return rc;
  }
  *out = L;
  return ISPH_SUCCESS;
}

int isph_nlist_info(const isph_nlist *nl, long long info[4]) {
  ISPH_REQUIRE(nl && info, "NULL argument");
  info[0] = nl->nlocal; info[1] = nl->nghost; info[2] = nl->nnz; info[3] = nl->fits32;
  return ISPH_SUCCESS;
}

int isph_nlist_get(isph_ctx *ctx, const isph_nlist *nl, double *x_all, int *owner_index, long long *neigh_ptr64, int *neigh_ptr,
                   int *neigh_idx, int on_device) {
  using namespace isph;
  ISPH_REQUIRE(ctx && nl, "NULL argument");
  ISPH_REQUIRE(!neigh_ptr || nl->fits32, "the list entries do not fit 32-bit offsets: take neigh_ptr64");
  const size_t nall = (size_t)nl->nlocal + (size_t)nl->nghost, n1 = (size_t)nl->nlocal + 1;
  ISPH_CHECK(nl_copy_out(ctx, x_all, (const double *)nl->x.p, nall * 3, on_device));
  ISPH_CHECK(nl_copy_out(ctx, owner_index, (const int *)nl->owner.p, nall, on_device));
  ISPH_CHECK(nl_copy_out(ctx, neigh_ptr64, (const long long *)nl->ptr64.p, n1, on_device));
  ISPH_CHECK(nl_copy_out(ctx, neigh_ptr, (const int *)nl->ptr32.p, n1, on_device));
  ISPH_CHECK(nl_copy_out(ctx, neigh_idx, (const int *)nl->idx.p, (size_t)nl->nnz, on_device));
  ISPH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  return ISPH_SUCCESS;
}

int isph_nlist_destroy(isph_ctx *ctx, isph_nlist *nl) {
  (void)ctx;
  if (!nl) return ISPH_SUCCESS;
  nl->release();
  delete nl;
  return ISPH_SUCCESS;
}

}  // extern "C"
