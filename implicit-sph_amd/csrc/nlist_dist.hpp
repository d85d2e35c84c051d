// nlist_dist.hpp -- what happens between two compute() calls on a brick of ranks, on the device: migration of the
// particles that left their sub-box (isph_migrate, LAMMPS' Comm::exchange), ghost atoms from the neighbouring ranks and
// from periodic images, the full neighbour list, the column map and the halo plan (isph_nlist_build_dist, Comm::borders +
// Neighbor::build + what Epetra's FillComplete derives), and the forward comm of per-atom arrays through that plan
// (isph_nlist_forward, forward_comm_pair; isph_nlist_forward_multi: several arrays in one exchange).
//
// Everything between ranks goes through comm.hpp: comm_exchange with a temporary isph_halo over the (at most 26) grid
// neighbours, comm_consensus for the failure flags.  Integers travel as doubles (exact below 2^53).  No kernel waits on
// another rank; order comes from the stream and the host calls.
//
// The slots.  A rank looks at its <= 26 grid offsets d in {-1, 0, 1}^3 \ 0.  Offset d_a on axis a leads to grid coordinate
// c_a + d_a, wrapped on a periodic axis with image shift s_a = -d_a when it crosses the boundary, and to nothing on a
// non-periodic outer face.  An owned particle is needed behind offset d when on every axis with d_a = -1
// x_a - flo_a < cut and on every axis with d_a = +1 x_a >= fhi_a - cut (the one-rank builder's form; flo / fhi the
// owner's faces).  The host lists the slots in ascending (sz, sy, sx): for one receiver the shifts of the slots that lead
// to it are distinct, so a particle's records for one receiver come out in ascending shift, and a sender's segment is
// sorted by (owner index, shift) without a sort.  With one rank on an axis the slots are the self-images of
// neighbours.hpp in its order.
//
// Stages of isph_nlist_build_dist (read-backs: offenders + per-segment record counts, the counts the peers send, the
// list's entry count, per-segment ghost / column / send counts):
//   1 k_dd_mask    wrap, ownership check, slot mask of every owned particle, records per (segment, particle)
//                  -> one exclusive scan over [segment][particle] = the position of every record in the send buffer
//   2 k_dd_pack    records (x + s P, owner index), segments of the off-rank receivers ascending, the self-images last
//   3 counts, then records, through comm_exchange; k_dd_unpack: owned + ghosts by (owner rank, owner index, shift)
//   4 nl_list_rows (neighbours.hpp stages 3 - 5, unchanged kernels)
//   5 prune: k_dd_mark, scans, k_dd_compact, k_dd_renumber; the flags of the survivors go back to the senders with the
//     reverse comm_exchange
//   6 k_dd_columns / k_dd_select: column map on the receiver, send lists on the sender -- both sides count the same
//     distinct (owner rank, owner index) pairs, so no all-gather is needed
// A rank that fails a check carries its rc to the next consensus, which stands before every exchange.
#pragma once
#include <algorithm>

#include "comm.hpp"
#include "neighbours.hpp"

struct isph_migrated {
  int nlocal = 0, nd = 0, ni = 0, nsent = 0, nrecv = 0;
  isph::DevBuf<double> x, fd;   // [nlocal][3], [nlocal][nd]
  isph::DevBuf<int> fi;         // [nlocal][ni]
  void release() { x.release(); fd.release(); fi.release(); }
};

namespace isph {

constexpr int kDdSlots = 26, kDdSegs = 27;

struct DdGeom {   // passed to the kernels by value
  int dim, nslots, nsegs, me;
  double lo[3], period[3], flo[3], fhi[3], cut;
  int periodic[3], open_lo[3], open_hi[3];   // open: a non-periodic outer face, no bound on that side
  signed char d[kDdSlots][3], s[kDdSlots][3];
  int seg[kDdSlots];             // segment of the send buffer the slot's records go to
  unsigned segmask[kDdSegs];     // the slots of a segment
};

struct DdSegs {   // ghost order: the segments by ascending owner rank (this rank's images among them)
  int nsegs;
  int gstart[kDdSegs + 1];   // first ghost of the segment
  int rank[kDdSegs];
  int src[kDdSegs];          // first record: in the receive buffer, or (self) in the send buffer
  int self;                  // index of the own segment, -1: none
};

struct DdAt { int m; int at[64]; };

// the decomposition as the host sees it
struct DdHost {
  DdGeom G;
  int pg[3], c[3];
  std::vector<double> faces[3];
  std::vector<int> peer;      // off-rank segments, ascending ranks: segment p < peer.size() goes to peer[p]
  int self_seg = -1;          // the last segment when there are self-images
};

inline int dd_rank_of(const int pg[3], const int c[3]) { return c[0] + pg[0] * (c[1] + pg[1] * c[2]); }

inline int dd_setup(isph_ctx *ctx, const isph_decomp *dc, double cut, bool need_cut, DdHost &D) {
  ISPH_REQUIRE(dc->dim == 2 || dc->dim == 3, "decomposition: dim must be 2 or 3");
  const int dim = dc->dim;
  long long prod = 1;
  for (int a = 0; a < 3; ++a) {
    ISPH_REQUIRE(dc->pgrid[a] >= 1 && dc->pgrid[a] <= 1 << 20, "decomposition: pgrid entries must be positive");
    ISPH_REQUIRE(a < dim || dc->pgrid[a] == 1, "decomposition: pgrid[2] must be 1 in 2-D");
    prod *= dc->pgrid[a];
    D.pg[a] = dc->pgrid[a];
  }
  const int nranks = comm_active(ctx) ? ctx->nranks : 1;
  ISPH_REQUIRE(prod == (long long)nranks, "decomposition: pgrid[0] * pgrid[1] * pgrid[2] differs from the number of ranks");
  ISPH_REQUIRE(!need_cut || cut > 0.0, "cut must be positive");
  DdGeom &G = D.G;
  memset(&G, 0, sizeof(G));
  G.dim = dim; G.cut = cut; G.me = comm_active(ctx) ? ctx->rank : 0;
  int r = G.me;
  for (int a = 0; a < 3; ++a) { D.c[a] = r % D.pg[a]; r /= D.pg[a]; }
  for (int a = 0; a < 3; ++a) {
    const int pg = D.pg[a];
    std::vector<double> &f = D.faces[a];
    f.assign((size_t)pg + 1, 0.0);
    G.lo[a] = a < dim ? dc->lo[a] : 0.0;
    const double hi = a < dim ? dc->hi[a] : 0.0;
    G.period[a] = hi - G.lo[a];
    G.periodic[a] = a < dim && dc->periodic[a] != 0;
    if (a >= dim) { G.flo[a] = G.fhi[a] = 0.0; G.open_lo[a] = G.open_hi[a] = 1; continue; }
    ISPH_REQUIRE(hi > G.lo[a], "decomposition: hi must exceed lo");
    if (dc->faces[a]) {
      for (int k = 0; k <= pg; ++k) f[(size_t)k] = dc->faces[a][k];
      ISPH_REQUIRE(f[0] == G.lo[a] && f[(size_t)pg] == hi, "decomposition: faces must start at lo and end at hi");
    } else {
      const double w = (hi - G.lo[a]) / pg;
      for (int k = 0; k < pg; ++k) f[(size_t)k] = G.lo[a] + k * w;
      f[(size_t)pg] = hi;
    }
    for (int k = 0; k < pg; ++k) {
      ISPH_REQUIRE(f[(size_t)k + 1] > f[(size_t)k], "decomposition: faces must ascend");
      if (need_cut && pg > 1) ISPH_REQUIRE(f[(size_t)k + 1] - f[(size_t)k] >= cut, "decomposition: a sub-box is narrower than the cut");
    }
    if (need_cut && pg == 1 && G.periodic[a]) ISPH_REQUIRE(hi - G.lo[a] >= 2.0 * cut, "a periodic axis is shorter than two cuts");
    G.flo[a] = f[(size_t)D.c[a]];
    G.fhi[a] = f[(size_t)D.c[a] + 1];
    G.open_lo[a] = !G.periodic[a] && D.c[a] == 0;
    G.open_hi[a] = !G.periodic[a] && D.c[a] == pg - 1;
  }
  // per axis: the offsets that lead somewhere, by ascending shift
  struct Opt { int d, s, tc; };
  std::vector<Opt> opt[3];
  for (int a = 0; a < 3; ++a) {
    for (int d = -1; d <= 1; ++d) {
      if (a >= dim && d != 0) continue;
      int tc = D.c[a] + d, s = 0;
      if (tc < 0) { if (!G.periodic[a]) continue; tc = D.pg[a] - 1; s = 1; }
      if (tc >= D.pg[a]) { if (!G.periodic[a]) continue; tc = 0; s = -1; }
      opt[a].push_back({d, s, tc});
    }
    std::stable_sort(opt[a].begin(), opt[a].end(), [](const Opt &p, const Opt &q) { return p.s < q.s; });
  }
  int srank[kDdSlots];
  std::vector<int> ranks;
  int ns = 0;
  for (const Opt &oz : opt[2])
    for (const Opt &oy : opt[1])
      for (const Opt &ox : opt[0]) {
        if (!ox.d && !oy.d && !oz.d) continue;
        const int tc[3] = {ox.tc, oy.tc, oz.tc};
        G.d[ns][0] = (signed char)ox.d; G.d[ns][1] = (signed char)oy.d; G.d[ns][2] = (signed char)oz.d;
        G.s[ns][0] = (signed char)ox.s; G.s[ns][1] = (signed char)oy.s; G.s[ns][2] = (signed char)oz.s;
        srank[ns] = dd_rank_of(D.pg, tc);
        if (srank[ns] != G.me) ranks.push_back(srank[ns]);
        ++ns;
      }
  G.nslots = ns;
  std::sort(ranks.begin(), ranks.end());
  ranks.erase(std::unique(ranks.begin(), ranks.end()), ranks.end());
  D.peer = ranks;
  D.self_seg = -1;
  G.nsegs = (int)ranks.size();
  for (int k = 0; k < ns; ++k)
    if (srank[k] == G.me) D.self_seg = (int)ranks.size();
  if (D.self_seg >= 0) G.nsegs = D.self_seg + 1;
  for (int k = 0; k < ns; ++k) {
    G.seg[k] = srank[k] == G.me ? D.self_seg : (int)(std::lower_bound(ranks.begin(), ranks.end(), srank[k]) - ranks.begin());
    G.segmask[G.seg[k]] |= 1u << k;
  }
  return ISPH_SUCCESS;
}

__device__ inline void dd_wrap(const DdGeom &G, const double *x, double *p) {
  for (int a = 0; a < 3; ++a) {
    p[a] = x[a];
    if (a < G.dim && G.periodic[a]) p[a] = nl_wrap(p[a], G.lo[a], G.period[a]);
  }
}

// cnt: [nsegs][n] records of particle i for segment p; bad: owned particles outside the sub-box (a count)
__global__ void k_dd_mask(int n, DdGeom G, const double *__restrict__ x, double *__restrict__ xw, unsigned *__restrict__ mask,
                          int *__restrict__ cnt, int *__restrict__ bad) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double p[3];
  dd_wrap(G, x + 3 * (size_t)i, p);
  bool low[3], high[3], out = false;
  for (int a = 0; a < 3; ++a) {
    xw[3 * (size_t)i + a] = p[a];
    low[a] = high[a] = false;
    if (a >= G.dim) continue;
    if ((!G.open_lo[a] && p[a] < G.flo[a]) || (!G.open_hi[a] && !(p[a] < G.fhi[a]))) out = true;
    low[a] = p[a] - G.flo[a] < G.cut;
    high[a] = p[a] >= G.fhi[a] - G.cut;
  }
  if (out) atomicAdd(bad, 1);   // a count: the order of arrival does not show
  unsigned m = 0;
  for (int k = 0; k < G.nslots; ++k) {
    bool ok = true;
    for (int a = 0; a < 3; ++a) ok = ok && (G.d[k][a] == 0 || (G.d[k][a] < 0 ? low[a] : high[a]));
    if (ok) m |= 1u << k;
  }
  mask[i] = m;
  for (int q = 0; q < G.nsegs; ++q) cnt[(size_t)q * n + i] = __popc(m & G.segmask[q]);
}

// rec: [records][4] = position of the ghost, owner index
__global__ void k_dd_pack(int n, DdGeom G, const double *__restrict__ xw, const unsigned *__restrict__ mask,
                          const int *__restrict__ off, double *__restrict__ rec) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned m = mask[i];
  if (!m) return;
  const double p0 = xw[3 * (size_t)i], p1 = xw[3 * (size_t)i + 1], p2 = xw[3 * (size_t)i + 2];
  for (int k = 0; k < G.nslots; ++k) {
    if (!(m >> k & 1u)) continue;
    const int q = G.seg[k];
    const size_t r = (size_t)off[(size_t)q * n + i] + (size_t)__popc(m & G.segmask[q] & ((1u << k) - 1u));
    // s is -1, 0 or 1: the product is exact, so the sum is rounded once whether or not it is fused
    rec[4 * r] = p0 + (double)G.s[k][0] * G.period[0];
    rec[4 * r + 1] = p1 + (double)G.s[k][1] * G.period[1];
    rec[4 * r + 2] = G.dim == 3 ? p2 + (double)G.s[k][2] * G.period[2] : 0.0;
    rec[4 * r + 3] = (double)i;
  }
}

__device__ inline int dd_seg_of(const DdSegs &S, int g) {
  int j = 0;
  while (j + 1 < S.nsegs && g >= S.gstart[j + 1]) ++j;
  return j;
}

__global__ void k_dd_unpack(int n, int nall, int me, DdSegs S, const double *__restrict__ xw, const double *__restrict__ sbuf,
                            const double *__restrict__ rbuf, double *__restrict__ x, int *__restrict__ owner, int *__restrict__ orank) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nall) return;
  if (i < n) {
    for (int a = 0; a < 3; ++a) x[3 * (size_t)i + a] = xw[3 * (size_t)i + a];
    owner[i] = i;
    orank[i] = me;
    return;
  }
  const int g = i - n, j = dd_seg_of(S, g);
  const double *r = (j == S.self ? sbuf : rbuf) + 4 * ((size_t)S.src[j] + (size_t)(g - S.gstart[j]));
  for (int a = 0; a < 3; ++a) x[3 * (size_t)i + a] = r[a];
  owner[i] = (int)r[3];
  orank[i] = S.rank[j];
}

__global__ void k_dd_mark(long long nnz, int n, const int *__restrict__ idx, int *__restrict__ keep) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nnz) return;
  const int j = idx[e];
  if (j >= n) keep[j - n] = 1;   // every writer stores the same value
}

__global__ void k_dd_fill_int(int n, int v, int *__restrict__ a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) a[i] = v;
}

// first[g]: kept off-rank ghost g opens a column -- no kept ghost before it has its (owner rank, owner index)
__global__ void k_dd_first(int n, int nghost, int me, const int *__restrict__ keep, const int *__restrict__ owner,
                           const int *__restrict__ orank, int *__restrict__ first) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= nghost) return;
  const int r = orank[n + g], o = owner[n + g];
  int f = keep[g] && r != me;
  for (int h = g - 1; f && h >= 0 && orank[n + h] == r && owner[n + h] == o; --h)
    if (keep[h]) f = 0;
  first[g] = f;
}

__global__ void k_dd_gather_at(DdAt A, const int *__restrict__ src, int *__restrict__ dst) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < A.m) dst[k] = src[A.at[k]];
}

// the surviving ghosts move up: position, owner, owner rank, column; the flags of the off-rank ghosts in the order of
// the receive buffer, for their senders
__global__ void k_dd_compact(int n, int nghost, int me, DdSegs S, const int *__restrict__ keep, const int *__restrict__ kpos,
                             const int *__restrict__ first, const int *__restrict__ cpos, const double *__restrict__ x0,
                             const int *__restrict__ owner0, const int *__restrict__ orank0, double *__restrict__ x,
                             int *__restrict__ owner, int *__restrict__ orank, int *__restrict__ colmap, double *__restrict__ flag) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n + nghost) return;
  if (i < n) {
    for (int a = 0; a < 3; ++a) x[3 * (size_t)i + a] = x0[3 * (size_t)i + a];
    owner[i] = i; orank[i] = me; colmap[i] = i;
    return;
  }
  const int g = i - n, k = keep[g];
  if (flag) {
    const int j = dd_seg_of(S, g);
    if (j != S.self) flag[(size_t)S.src[j] + (size_t)(g - S.gstart[j])] = k ? 1.0 : 0.0;
  }
  if (!k) return;
  const size_t t = (size_t)n + (size_t)kpos[g];
  for (int a = 0; a < 3; ++a) x[3 * t + a] = x0[3 * (size_t)i + a];
  owner[t] = owner0[i];
  orank[t] = orank0[i];
  colmap[t] = orank0[i] == me ? owner0[i] : n + cpos[g] + first[g] - 1;
}

__global__ void k_dd_renumber(long long nnz, int n, const int *__restrict__ kpos, int *__restrict__ idx) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nnz) return;
  const int j = idx[e];
  if (j >= n) idx[e] = n + kpos[j - n];
}

// sel[r]: record r of an off-rank segment opens an entry of the send list -- it survived on the receiver (flag, NULL: all
// did) and no surviving record before it in its segment has its owner index.  segstart: [np + 1] in P.at
__global__ void k_dd_select(int nrec, DdAt P, const double *__restrict__ rec, const double *__restrict__ flag, int *__restrict__ sel) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= nrec) return;
  int j = 0;
  while (j + 1 < P.m - 1 && r >= P.at[j + 1]) ++j;
  const int b = P.at[j];
  const double o = rec[4 * (size_t)r + 3];
  int s = !flag || flag[r] != 0.0;
  for (int h = r - 1; s && h >= b && rec[4 * (size_t)h + 3] == o; --h)
    if (!flag || flag[h] != 0.0) s = 0;
  sel[r] = s;
}

__global__ void k_dd_send_idx(int nrec, const double *__restrict__ rec, const int *__restrict__ sel, const int *__restrict__ spos,
                              int *__restrict__ send_idx) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < nrec && sel[r]) send_idx[spos[r]] = (int)rec[4 * (size_t)r + 3];
}

inline dim3 dd_grid(long long n) { return dim3((unsigned)((n + kBlock - 1) / kBlock)); }

// a temporary isph_halo over the off-rank segments with the given counts per peer
inline void dd_make_halo(const std::vector<int> &peer, const std::vector<int> &nsend, const std::vector<int> &nrecv, isph_halo &H) {
  H.npeers = (int)peer.size();
  H.peer = peer;
  H.send_ptr.assign(peer.size() + 1, 0);
  H.recv_ptr.assign(peer.size() + 1, 0);
  for (size_t p = 0; p < peer.size(); ++p) {
    H.send_ptr[p + 1] = H.send_ptr[p] + nsend[p];
    H.recv_ptr[p + 1] = H.recv_ptr[p] + nrecv[p];
  }
  H.nsend = H.send_ptr[peer.size()];
  H.nrecv = H.recv_ptr[peer.size()];
}

// how many records every peer sends: one number each way
inline int dd_exchange_counts(isph_ctx *ctx, const std::vector<int> &peer, const std::vector<int> &nsend, std::vector<int> &nrecv) {
  const size_t np = peer.size();
  nrecv.assign(np, 0);
  if (np == 0) return ISPH_SUCCESS;
  isph_halo H;
  dd_make_halo(peer, std::vector<int>(np, 1), std::vector<int>(np, 1), H);
  std::vector<double> h(np);
  for (size_t p = 0; p < np; ++p) h[p] = (double)nsend[p];
  DevTmp<double> ds, dr;
  ISPH_CHECK(ds.reserve(np));
  ISPH_CHECK(dr.reserve(np));
  ISPH_CHECK_HIP(hipMemcpyAsync(ds.p, h.data(), sizeof(double) * np, hipMemcpyHostToDevice, ctx->stream));
  ISPH_CHECK(comm_exchange(ctx, H, ds.p, dr.p, 1, false, ctx->stream));
  ISPH_CHECK_HIP(hipMemcpyAsync(h.data(), dr.p, sizeof(double) * np, hipMemcpyDeviceToHost, ctx->stream));
  ISPH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  for (size_t p = 0; p < np; ++p) {
    ISPH_REQUIRE(h[p] >= 0.0 && h[p] < (double)INT_MAX, "a peer announced an impossible count");
    nrecv[p] = (int)h[p];
  }
  return ISPH_SUCCESS;
}

// src[A.at[k]] for k < A.m, read back
inline int dd_read_at(isph_ctx *ctx, const DdAt &A, const int *src, int *out) {
  DevTmp<int> d;
  ISPH_CHECK(d.reserve((size_t)A.m));
  hipLaunchKernelGGL(k_dd_gather_at, dim3(1), dim3(64), 0, ctx->stream, A, src, d.p);
  ISPH_CHECK_HIP(hipMemcpyAsync(out, d.p, sizeof(int) * (size_t)A.m, hipMemcpyDeviceToHost, ctx->stream));
  ISPH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  ISPH_CHECK_HIP(hipGetLastError());
  return ISPH_SUCCESS;
}

template <class T>
inline int dd_stage_in(isph_ctx *ctx, const T *src, size_t count, int on_device, DevTmp<T> &tmp, const T **dev) {
  *dev = src;
  if (on_device || count == 0) return ISPH_SUCCESS;
  ISPH_REQUIRE(!is_device_pointer(src), "on_device = 0 but an input is device memory");
  ISPH_CHECK(tmp.reserve(count));
  ISPH_CHECK_HIP(hipMemcpyAsync(tmp.p, src, sizeof(T) * count, hipMemcpyHostToDevice, ctx->stream));
  *dev = tmp.p;
  return ISPH_SUCCESS;
}

constexpr const char *kDdBroken = "nlist: the consensus all-reduce failed";

struct DdBuild {   // what the stages of one build share
  DdHost D;
  int n = 0, nseg = 0, nrec_off = 0, nrec_self = 0, nghost = 0;
  std::vector<int> segcount, nrecv;   // records per segment of the send buffer; records every peer sends
  DevTmp<double> xin, xw, sbuf, rbuf, flag, sflag;
  DevTmp<unsigned> mask;
  DevTmp<int> cnt, off;
  DdSegs S;
};

inline int dd_stage_select(isph_ctx *ctx, int n, const double *x, int on_device, DdBuild &B) {
  hipStream_t st = ctx->stream;
  const DdGeom &G = B.D.G;
  const int nseg = G.nsegs;
  B.n = n; B.nseg = nseg;
  B.segcount.assign((size_t)nseg, 0);
  if (n == 0) return ISPH_SUCCESS;
  const double *dx = nullptr;
  ISPH_CHECK(dd_stage_in(ctx, x, (size_t)n * 3, on_device, B.xin, &dx));
  const size_t nc = (size_t)nseg * (size_t)n + 1;
  ISPH_REQUIRE(nc < (size_t)INT_MAX, "too many particles");
  DevTmp<int> bad;
  ISPH_CHECK(bad.reserve(1));
  ISPH_CHECK(B.xw.reserve((size_t)n * 3));
  ISPH_CHECK(B.mask.reserve((size_t)n));
  ISPH_CHECK(B.cnt.reserve(nc));
  ISPH_CHECK(B.off.reserve(nc));
  ISPH_CHECK_HIP(hipMemsetAsync(bad.p, 0, sizeof(int), st));
  ISPH_CHECK_HIP(hipMemsetAsync(B.cnt.p + (nc - 1), 0, sizeof(int), st));
  hipLaunchKernelGGL(k_dd_mask, dd_grid(n), dim3(kBlock), 0, st, n, G, dx, B.xw.p, B.mask.p, B.cnt.p, bad.p);
  ISPH_CHECK(nl_exclusive_scan<int>(st, B.cnt.p, B.off.p, nc));
  DdAt A;
  A.m = nseg + 1;
  for (int q = 0; q <= nseg; ++q) A.at[q] = (int)((size_t)q * (size_t)n);
  int h[kDdSegs + 2], nbad = 0;
  ISPH_CHECK_HIP(hipMemcpyAsync(&nbad, bad.p, sizeof(int), hipMemcpyDeviceToHost, st));
  ISPH_CHECK(dd_read_at(ctx, A, B.off.p, h));
  if (nbad != 0) {
    char msg[128];
    snprintf(msg, sizeof(msg), "isph_nlist_build_dist: %d owned particles lie outside the rank's sub-box", nbad);
    return fail(msg, __FILE__, __LINE__);
  }
  for (int q = 0; q < nseg; ++q) B.segcount[(size_t)q] = h[q + 1] - h[q];
  ISPH_REQUIRE(h[nseg] >= 0, "record count failed");
  return ISPH_SUCCESS;
}

inline int dd_stage_pack(isph_ctx *ctx, DdBuild &B) {
  const int np = (int)B.D.peer.size();
  B.nrec_off = 0;
  for (int p = 0; p < np; ++p) B.nrec_off += B.segcount[(size_t)p];
  B.nrec_self = B.D.self_seg >= 0 ? B.segcount[(size_t)B.D.self_seg] : 0;
  const size_t nrec = (size_t)B.nrec_off + (size_t)B.nrec_self;
  ISPH_CHECK(B.sbuf.reserve(4 * (nrec > 0 ? nrec : 1)));
  if (B.n > 0 && nrec > 0)
    hipLaunchKernelGGL(k_dd_pack, dd_grid(B.n), dim3(kBlock), 0, ctx->stream, B.n, B.D.G, (const double *)B.xw.p,
                       (const unsigned *)B.mask.p, (const int *)B.off.p, B.sbuf.p);
  ISPH_CHECK_HIP(hipGetLastError());
  return ISPH_SUCCESS;
}

// the ghost order from the counts: segments by ascending owner rank
inline int dd_stage_segments(DdBuild &B) {
  const std::vector<int> &peer = B.D.peer;
  const int np = (int)peer.size(), me = B.D.G.me;
  DdSegs &S = B.S;
  memset(&S, 0, sizeof(S));
  S.self = -1;
  long long g = 0;
  int j = 0, rstart = 0;
  bool self_done = B.D.self_seg < 0;
  for (int p = 0; p <= np; ++p) {
    if (!self_done && (p == np || peer[(size_t)p] > me)) {
      S.self = j; S.gstart[j] = (int)g; S.rank[j] = me; S.src[j] = B.nrec_off;
      g += B.nrec_self; ++j; self_done = true;
    }
    if (p == np) break;
    S.gstart[j] = (int)g; S.rank[j] = peer[(size_t)p]; S.src[j] = rstart;
    g += B.nrecv[(size_t)p]; rstart += B.nrecv[(size_t)p]; ++j;
  }
  S.nsegs = j;
  S.gstart[j] = (int)g;
  ISPH_REQUIRE(g + B.n < (long long)INT_MAX, "too many particles");
  B.nghost = (int)g;
  return ISPH_SUCCESS;
}

inline int dd_stage_ghosts(isph_ctx *ctx, DdBuild &B, isph_nlist &L) {
  const int n = B.n, nall = n + B.nghost;
  L.nghost = B.nghost;
  ISPH_CHECK(L.x.reserve((size_t)(nall > 0 ? nall : 1) * 3));
  ISPH_CHECK(L.owner.reserve((size_t)(nall > 0 ? nall : 1)));
  ISPH_CHECK(L.orank.reserve((size_t)(nall > 0 ? nall : 1)));
  if (nall > 0)
    hipLaunchKernelGGL(k_dd_unpack, dd_grid(nall), dim3(kBlock), 0, ctx->stream, n, nall, B.D.G.me, B.S, (const double *)B.xw.p,
                       (const double *)B.sbuf.p, (const double *)B.rbuf.p, L.x.p, L.owner.p, L.orank.p);
  ISPH_CHECK_HIP(hipGetLastError());
  return ISPH_SUCCESS;
}

inline int dd_stage_list(isph_ctx *ctx, double cut, DdBuild &B, isph_nlist &L) {
  hipStream_t st = ctx->stream;
  const int n = B.n;
  ISPH_CHECK(L.ptr64.reserve((size_t)n + 1));
  if (n > 0) return nl_list_rows(ctx, L.dim, n, n + B.nghost, cut, L);
  ISPH_CHECK_HIP(hipMemsetAsync(L.ptr64.p, 0, sizeof(long long), st));
  ISPH_CHECK(L.ptr32.reserve(1));
  ISPH_CHECK_HIP(hipMemsetAsync(L.ptr32.p, 0, sizeof(int), st));
  ISPH_CHECK(L.idx.reserve(1));
  ISPH_CHECK_HIP(hipStreamSynchronize(st));
  L.nnz = 0; L.fits32 = 1;
  return ISPH_SUCCESS;
}

// marks, scans, compaction; fills L.colmap, B.flag (prune) and the receive side of the plan (recv counts per peer)
inline int dd_stage_prune(isph_ctx *ctx, int prune, DdBuild &B, isph_nlist &L, std::vector<int> &ncol_from) {
  hipStream_t st = ctx->stream;
  const int n = B.n, ng = B.nghost, me = B.D.G.me, np = (int)B.D.peer.size();
  ncol_from.assign((size_t)np, 0);
  L.ncol = n; L.noffrank = 0;
  DevTmp<int> keep, first, pos;   // pos: the exclusive scans of keep and of first, one behind the other
  ISPH_CHECK(keep.reserve((size_t)ng + 1));
  ISPH_CHECK(first.reserve((size_t)ng + 1));
  ISPH_CHECK(pos.reserve(2 * ((size_t)ng + 1)));
  int *const kpos = pos.p, *const cpos = pos.p + ((size_t)ng + 1);
  ISPH_CHECK_HIP(hipMemsetAsync(keep.p, 0, sizeof(int) * ((size_t)ng + 1), st));
  ISPH_CHECK_HIP(hipMemsetAsync(first.p, 0, sizeof(int) * ((size_t)ng + 1), st));
  if (ng > 0) {
    if (prune) {
      if (L.nnz > 0) hipLaunchKernelGGL(k_dd_mark, dd_grid(L.nnz), dim3(kBlock), 0, st, L.nnz, n, (const int *)L.idx.p, keep.p);
    } else {
      hipLaunchKernelGGL(k_dd_fill_int, dd_grid(ng), dim3(kBlock), 0, st, ng, 1, keep.p);
    }
    hipLaunchKernelGGL(k_dd_first, dd_grid(ng), dim3(kBlock), 0, st, n, ng, me, (const int *)keep.p, (const int *)L.owner.p,
                       (const int *)L.orank.p, first.p);
  }
  ISPH_CHECK(nl_exclusive_scan<int>(st, keep.p, kpos, (size_t)ng + 1));
  ISPH_CHECK(nl_exclusive_scan<int>(st, first.p, cpos, (size_t)ng + 1));
  // kept ghosts and columns at the segment boundaries: one read-back
  const DdSegs &S = B.S;
  DdAt A;
  A.m = 2 * (S.nsegs + 1);
  for (int j = 0; j <= S.nsegs; ++j) { A.at[j] = S.gstart[j]; A.at[S.nsegs + 1 + j] = ng + 1 + S.gstart[j]; }
  int hb[2 * (kDdSegs + 2)];
  ISPH_CHECK(dd_read_at(ctx, A, pos.p, hb));
  const int *hk = hb, *hc = hb + S.nsegs + 1;
  const int nkeep = hk[S.nsegs];
  ISPH_REQUIRE(nkeep >= 0 && nkeep <= ng, "ghost count failed");
  for (int j = 0, p = 0; j < S.nsegs; ++j) {
    if (j == S.self) continue;
    ncol_from[(size_t)p++] = hc[j + 1] - hc[j];
    L.noffrank += hk[j + 1] - hk[j];
  }
  L.ncol = n + hc[S.nsegs];
  const int nall = n + nkeep;
  if (prune) ISPH_CHECK(B.flag.reserve((size_t)(B.S.gstart[S.nsegs] > 0 ? B.S.gstart[S.nsegs] : 1)));
  DevBuf<double> x1;
  DevBuf<int> owner1, orank1;
  int rc = x1.reserve((size_t)(nall > 0 ? nall : 1) * 3);
  if (rc == ISPH_SUCCESS) rc = owner1.reserve((size_t)(nall > 0 ? nall : 1));
  if (rc == ISPH_SUCCESS) rc = orank1.reserve((size_t)(nall > 0 ? nall : 1));
  if (rc == ISPH_SUCCESS) rc = L.colmap.reserve((size_t)(nall > 0 ? nall : 1));
  if (rc != ISPH_SUCCESS) { x1.release(); owner1.release(); orank1.release(); return rc; }
  if (n + ng > 0)
    hipLaunchKernelGGL(k_dd_compact, dd_grid(n + ng), dim3(kBlock), 0, st, n, ng, me, S, (const int *)keep.p, (const int *)kpos,
                       (const int *)first.p, (const int *)cpos, (const double *)L.x.p, (const int *)L.owner.p,
                       (const int *)L.orank.p, x1.p, owner1.p, orank1.p, L.colmap.p, prune ? B.flag.p : (double *)nullptr);
  if (nkeep != ng && L.nnz > 0)
    hipLaunchKernelGGL(k_dd_renumber, dd_grid(L.nnz), dim3(kBlock), 0, st, L.nnz, n, (const int *)kpos, L.idx.p);
  std::swap(L.x, x1); std::swap(L.owner, owner1); std::swap(L.orank, orank1);
  x1.release(); owner1.release(); orank1.release();
  L.nghost = nkeep;
  ISPH_CHECK_HIP(hipStreamSynchronize(st));
  ISPH_CHECK_HIP(hipGetLastError());
  return ISPH_SUCCESS;
}

// the send side of the plan: distinct surviving owner indices per peer
inline int dd_stage_send_lists(isph_ctx *ctx, bool flags, DdBuild &B, isph_nlist &L, std::vector<int> &nsend_to) {
  hipStream_t st = ctx->stream;
  const int np = (int)B.D.peer.size(), nrec = B.nrec_off;
  nsend_to.assign((size_t)np, 0);
  ISPH_CHECK(L.halo.send_idx.reserve(1));
  if (nrec == 0) return ISPH_SUCCESS;
  DdAt P;
  P.m = np + 1;
  P.at[0] = 0;
  for (int p = 0; p < np; ++p) P.at[p + 1] = P.at[p] + B.segcount[(size_t)p];
  DevTmp<int> sel, spos;
  ISPH_CHECK(sel.reserve((size_t)nrec + 1));
  ISPH_CHECK(spos.reserve((size_t)nrec + 1));
  ISPH_CHECK_HIP(hipMemsetAsync(sel.p + nrec, 0, sizeof(int), st));
  hipLaunchKernelGGL(k_dd_select, dd_grid(nrec), dim3(kBlock), 0, st, nrec, P, (const double *)B.sbuf.p,
                     flags ? (const double *)B.sflag.p : (const double *)nullptr, sel.p);
  ISPH_CHECK(nl_exclusive_scan<int>(st, sel.p, spos.p, (size_t)nrec + 1));
  int h[kDdSegs + 2];
  ISPH_CHECK(dd_read_at(ctx, P, spos.p, h));
  for (int p = 0; p < np; ++p) nsend_to[(size_t)p] = h[p + 1] - h[p];
  ISPH_REQUIRE(h[np] >= 0 && h[np] <= nrec, "send count failed");
  ISPH_CHECK(L.halo.send_idx.reserve((size_t)(h[np] > 0 ? h[np] : 1)));
  hipLaunchKernelGGL(k_dd_send_idx, dd_grid(nrec), dim3(kBlock), 0, st, nrec, (const double *)B.sbuf.p, (const int *)sel.p,
                     (const int *)spos.p, L.halo.send_idx.p);
  ISPH_CHECK_HIP(hipStreamSynchronize(st));
  ISPH_CHECK_HIP(hipGetLastError());
  return ISPH_SUCCESS;
}

inline int nlist_build_dist(isph_ctx *ctx, const isph_decomp *dc, int nlocal, const double *x, double cut, int prune, int on_device,
                            isph_nlist &L) {
  const bool dist = comm_active(ctx) && ctx->nranks > 1;
  DdBuild B;
  L.dist = 1; L.dim = dc->dim; L.nlocal = nlocal;
  // 1. the decomposition, the records of every owned particle
  int rc = dd_setup(ctx, dc, cut, true, B.D);
  if (rc == ISPH_SUCCESS && !(nlocal >= 0 && nlocal <= INT_MAX / 32)) rc = fail("nlocal out of range", __FILE__, __LINE__);
  if (rc == ISPH_SUCCESS) rc = dd_stage_select(ctx, nlocal, x, on_device, B);
  // 2. the send buffer
  if (rc == ISPH_SUCCESS) rc = dd_stage_pack(ctx, B);
  if (!comm_consensus(ctx, dist, "nlist", kDdBroken, nullptr, 0, rc)) return rc;
  // 3. counts and records
  const std::vector<int> &peer = B.D.peer;
  const size_t np = peer.size();
  std::vector<int> nsend(B.segcount.begin(), B.segcount.begin() + (long)np);
  ISPH_CHECK(dd_exchange_counts(ctx, peer, nsend, B.nrecv));
  rc = dd_stage_segments(B);
  isph_halo H;
  dd_make_halo(peer, nsend, B.nrecv, H);
  if (rc == ISPH_SUCCESS) rc = B.rbuf.reserve(4 * (size_t)(H.nrecv > 0 ? H.nrecv : 1));
  if (!comm_consensus(ctx, dist, "nlist", kDdBroken, nullptr, 0, rc)) return rc;
  ISPH_CHECK(comm_exchange(ctx, H, B.sbuf.p, B.rbuf.p, 4, false, ctx->stream));
  rc = dd_stage_ghosts(ctx, B, L);
  // 4. the list
  if (rc == ISPH_SUCCESS) rc = dd_stage_list(ctx, cut, B, L);
  // 5. prune, column map
  std::vector<int> ncol_from, nsend_to;
  if (rc == ISPH_SUCCESS) rc = dd_stage_prune(ctx, prune, B, L, ncol_from);
  const bool flags = prune != 0 && np > 0;
  if (rc == ISPH_SUCCESS && flags) rc = B.sflag.reserve((size_t)(H.nsend > 0 ? H.nsend : 1));
  if (!comm_consensus(ctx, dist, "nlist", kDdBroken, nullptr, 0, rc)) return rc;
  if (flags) ISPH_CHECK(comm_exchange(ctx, H, B.flag.p, B.sflag.p, 1, /*reverse=*/true, ctx->stream));
  // 6. the send lists, the plan
  rc = dd_stage_send_lists(ctx, flags, B, L, nsend_to);
  if (!comm_consensus(ctx, dist, "nlist", kDdBroken, nullptr, 0, rc)) return rc;
  std::vector<int> pp, ps, pr;
  for (size_t p = 0; p < np; ++p)
    if (nsend_to[p] > 0 || ncol_from[p] > 0) { pp.push_back(peer[p]); ps.push_back(nsend_to[p]); pr.push_back(ncol_from[p]); }
  dd_make_halo(pp, ps, pr, L.halo);
  return ISPH_SUCCESS;
}

// ---- forward comm -------------------------------------------------------------------------------------------------------

template <class T>
__global__ void k_dd_fwd_pack(long long nelem, int ncomp, const int *__restrict__ send_idx, const T *__restrict__ a, double *__restrict__ sbuf) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nelem) return;
  const long long k = e / ncomp;
  sbuf[e] = (double)a[(long long)send_idx[k] * ncomp + (e - k * ncomp)];
}

template <class T>
__global__ void k_dd_fwd_gather(long long nelem, int ncomp, int n, int ncol, const int *__restrict__ colmap, const double *__restrict__ rbuf,
                                T *__restrict__ a) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nelem) return;
  const long long g = e / ncomp, c = e - g * ncomp;
  const int col = colmap[n + g];
  if (col < 0 || col >= ncol) return;   // never for a map this library made; keeps the reads in bounds
  a[((long long)n + g) * ncomp + c] = col < n ? a[(long long)col * ncomp + c] : (T)rbuf[(long long)(col - n) * ncomp + c];
}

template <class T>
inline int nlist_forward(isph_ctx *ctx, const isph_nlist *nl, int ncomp, T *a, int on_device) {
  hipStream_t st = ctx->stream;
  ISPH_REQUIRE(nl->dist, "isph_nlist_forward: the list was not built by isph_nlist_build_dist");
  ISPH_REQUIRE(ncomp >= 1, "isph_nlist_forward: ncomp must be positive");
  const int n = nl->nlocal, ng = nl->nghost;
  const size_t nall = (size_t)n + (size_t)ng;
  const isph_halo &H = nl->halo;
  ISPH_REQUIRE(a || nall == 0, "NULL argument");
  DevTmp<T> tmp;
  T *da = a;
  if (!on_device && nall > 0) {
    ISPH_REQUIRE(!is_device_pointer(a), "on_device = 0 but a is device memory");
    ISPH_CHECK(tmp.reserve(nall * (size_t)ncomp));
    ISPH_CHECK_HIP(hipMemcpyAsync(tmp.p, a, sizeof(T) * (size_t)n * ncomp, hipMemcpyHostToDevice, st));
    da = tmp.p;
  }
  DevTmp<double> sbuf, rbuf;
  ISPH_CHECK(sbuf.reserve((size_t)(H.nsend > 0 ? H.nsend : 1) * ncomp));
  ISPH_CHECK(rbuf.reserve((size_t)(H.nrecv > 0 ? H.nrecv : 1) * ncomp));
  const long long ns = (long long)H.nsend * ncomp, ne = (long long)ng * ncomp;
  if (ns > 0)
    hipLaunchKernelGGL(k_dd_fwd_pack<T>, dd_grid(ns), dim3(kBlock), 0, st, ns, ncomp, (const int *)H.send_idx.p, (const T *)da, sbuf.p);
  ISPH_CHECK(comm_exchange(ctx, H, sbuf.p, rbuf.p, ncomp, false, st));
  if (ne > 0)
    hipLaunchKernelGGL(k_dd_fwd_gather<T>, dd_grid(ne), dim3(kBlock), 0, st, ne, ncomp, n, nl->ncol, (const int *)nl->colmap.p,
                       (const double *)rbuf.p, da);
  if (!on_device && ng > 0)
    ISPH_CHECK_HIP(hipMemcpyAsync(a + (size_t)n * ncomp, da + (size_t)n * ncomp, sizeof(T) * (size_t)ng * ncomp, hipMemcpyDeviceToHost, st));
  ISPH_CHECK_HIP(hipStreamSynchronize(st));
  ISPH_CHECK_HIP(hipGetLastError());
  return ISPH_SUCCESS;
}

// several per-atom arrays in ONE exchange (PairISPH::pack_forward_comm sends several fields per message): a record of
// width = sum of ncomp doubles per listed atom, the arrays' components one behind the other; ints travel as doubles
constexpr int kFwdMaxArrays = 8;

struct FwdMulti {   // passed to the kernels by value
  int narr, width;
  void *a[kFwdMaxArrays];
  int ncomp[kFwdMaxArrays], is_int[kFwdMaxArrays];
  int off[kFwdMaxArrays + 1];   // first component of array j in the record
};

__device__ __forceinline__ int fwd_array_of(const FwdMulti &F, int c) {
  int j = 0;
  while (j + 1 < F.narr && c >= F.off[j + 1]) ++j;
  return j;
}

// one thread per double of the send buffer: consecutive lanes write consecutive doubles of a record
__global__ __launch_bounds__(kBlock) void k_dd_fwd_pack_multi(long long nelem, FwdMulti F, const int *__restrict__ send_idx,
                                                              double *__restrict__ sbuf) {
  const long long e = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (e >= nelem) return;
  const long long k = e / F.width;
  const int c = (int)(e - k * F.width), j = fwd_array_of(F, c);
  const long long src = (long long)send_idx[k] * F.ncomp[j] + (c - F.off[j]);
  sbuf[e] = F.is_int[j] ? (double)static_cast<const int *>(F.a[j])[src] : static_cast<const double *>(F.a[j])[src];
}

// one thread per double of a ghost's record: from the owner's row on this rank (a self-image) or from the receive buffer
__global__ __launch_bounds__(kBlock) void k_dd_fwd_gather_multi(long long nelem, FwdMulti F, int n, int ncol,
                                                                const int *__restrict__ colmap, const double *__restrict__ rbuf) {
  const long long e = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (e >= nelem) return;
  const long long g = e / F.width;
  const int c = (int)(e - g * F.width), j = fwd_array_of(F, c), nc = F.ncomp[j], cc = c - F.off[j];
  const int col = colmap[n + g];
  if (col < 0 || col >= ncol) return;   // never for a map this library made; keeps the reads in bounds
  const long long dst = ((long long)n + g) * nc + cc;
  if (F.is_int[j]) {
    int *a = static_cast<int *>(F.a[j]);
    a[dst] = col < n ? a[(long long)col * nc + cc] : (int)rbuf[(long long)(col - n) * F.width + c];
  } else {
    double *a = static_cast<double *>(F.a[j]);
    a[dst] = col < n ? a[(long long)col * nc + cc] : rbuf[(long long)(col - n) * F.width + c];
  }
}

// agree: the caller's arguments are checked and staged, then a consensus stands before the exchange, so a rank whose
// arguments are refused fails its peers with it (the stand-alone entry point).  The driver passes its own arrays and has
// its consensus behind it: no all-reduce of its own
inline int nlist_forward_multi(isph_ctx *ctx, const isph_nlist *nl, int narrays, const isph_fwd_array *arr, int on_device,
                               bool agree) {
  hipStream_t st = ctx->stream;
  const int n = nl->nlocal, ng = nl->nghost;
  const size_t nall = (size_t)n + (size_t)ng;
  const isph_halo &H = nl->halo;
  FwdMulti F;
  memset(&F, 0, sizeof(F));
  DevTmp<double> td[kFwdMaxArrays], sbuf, rbuf;
  DevTmp<int> ti[kFwdMaxArrays];
  auto local = [&]() -> int {
    ISPH_REQUIRE(nl->dist, "isph_nlist_forward_multi: the list was not built by isph_nlist_build_dist");
    ISPH_REQUIRE(narrays >= 1 && narrays <= kFwdMaxArrays && arr, "isph_nlist_forward_multi: 1 to 8 arrays are taken");
    F.narr = narrays;
    for (int j = 0; j < narrays; ++j) {
      ISPH_REQUIRE(arr[j].ncomp >= 1 && arr[j].ncomp <= 64, "isph_nlist_forward_multi: ncomp must be 1 .. 64");
      ISPH_REQUIRE(arr[j].a || nall == 0, "NULL argument");
      F.ncomp[j] = arr[j].ncomp; F.is_int[j] = arr[j].is_int != 0; F.off[j + 1] = F.off[j] + arr[j].ncomp;
      F.a[j] = arr[j].a;
      if (!on_device && nall > 0) {
        ISPH_REQUIRE(!is_device_pointer(arr[j].a), "on_device = 0 but an array is device memory");
        const size_t own = (size_t)n * (size_t)arr[j].ncomp, all = nall * (size_t)arr[j].ncomp;
        if (F.is_int[j]) {
          ISPH_CHECK(ti[j].reserve(all));
          ISPH_CHECK_HIP(hipMemcpyAsync(ti[j].p, arr[j].a, sizeof(int) * own, hipMemcpyHostToDevice, st));
          F.a[j] = ti[j].p;
        } else {
          ISPH_CHECK(td[j].reserve(all));
          ISPH_CHECK_HIP(hipMemcpyAsync(td[j].p, arr[j].a, sizeof(double) * own, hipMemcpyHostToDevice, st));
          F.a[j] = td[j].p;
        }
      }
    }
    F.width = F.off[narrays];
    ISPH_CHECK(sbuf.reserve((size_t)(H.nsend > 0 ? H.nsend : 1) * F.width));
    ISPH_CHECK(rbuf.reserve((size_t)(H.nrecv > 0 ? H.nrecv : 1) * F.width));
    return ISPH_SUCCESS;
  };
  int rc = local();
  if (agree) (void)comm_consensus(ctx, comm_active(ctx) && ctx->nranks > 1, "isph_nlist_forward_multi", kDdBroken, nullptr, 0, rc);
  ISPH_CHECK(rc);
  const long long ns = (long long)H.nsend * F.width, ne = (long long)ng * F.width;
  if (ns > 0)
    hipLaunchKernelGGL(k_dd_fwd_pack_multi, dd_grid(ns), dim3(kBlock), 0, st, ns, F, (const int *)H.send_idx.p, sbuf.p);
  ISPH_CHECK(comm_exchange(ctx, H, sbuf.p, rbuf.p, F.width, false, st));
  if (ne > 0)
    hipLaunchKernelGGL(k_dd_fwd_gather_multi, dd_grid(ne), dim3(kBlock), 0, st, ne, F, n, nl->ncol, (const int *)nl->colmap.p,
                       (const double *)rbuf.p);
  if (!on_device && ng > 0)
    for (int j = 0; j < narrays; ++j) {
      const size_t own = (size_t)n * (size_t)arr[j].ncomp, gh = (size_t)ng * (size_t)arr[j].ncomp;
      if (F.is_int[j]) ISPH_CHECK_HIP(hipMemcpyAsync((int *)arr[j].a + own, ti[j].p + own, sizeof(int) * gh, hipMemcpyDeviceToHost, st));
      else ISPH_CHECK_HIP(hipMemcpyAsync((double *)arr[j].a + own, td[j].p + own, sizeof(double) * gh, hipMemcpyDeviceToHost, st));
    }
  ISPH_CHECK_HIP(hipStreamSynchronize(st));
  ISPH_CHECK_HIP(hipGetLastError());
  return ISPH_SUCCESS;
}

// ---- migration ----------------------------------------------------------------------------------------------------------

struct MgGeom {
  int dim, nsegs, me;            // segment 0: the stayers, then the off-rank peers ascending
  double lo[3], period[3];
  int periodic[3], pg[3], c[3];
  int foff[3];                   // faces of axis a at faces[foff[a] .. foff[a] + pg[a]]
  int seg_of[27];                // segment of the grid offset (dz + 1) * 9 + (dy + 1) * 3 + dx + 1, -1: nowhere
};

// dest[i]: the segment particle i goes to, -1: farther than one sub-box; cnt [nsegs][n]
__global__ void k_mg_dest(int n, MgGeom G, const double *__restrict__ faces, const double *__restrict__ x, double *__restrict__ xw,
                          int *__restrict__ dest, int *__restrict__ cnt, int *__restrict__ far) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int code = 0, mul = 1;
  bool ok = true;
  for (int a = 0; a < 3; ++a) {
    double p = x[3 * (size_t)i + a];
    if (a < G.dim && G.periodic[a]) p = nl_wrap(p, G.lo[a], G.period[a]);
    xw[3 * (size_t)i + a] = p;
    int d = 0;
    if (a < G.dim) {
      const double *f = faces + G.foff[a];
      const int pg = G.pg[a];
      int t = 0;                                  // f[t] <= p < f[t + 1]; beyond an outer face: the outer cell
      while (t + 1 < pg && p >= f[t + 1]) ++t;
      d = t - G.c[a];
      if (G.periodic[a] && pg > 1) {
        if (t == (G.c[a] + 1) % pg) d = 1;
        else if (t == (G.c[a] + pg - 1) % pg) d = -1;
      }
      if (d < -1 || d > 1) ok = false;
    }
    code += (d + 1) * mul;
    mul *= 3;
  }
  const int q = ok ? G.seg_of[code] : -1;
  if (q < 0) atomicAdd(far, 1);   // a count: the order of arrival does not show
  dest[i] = q;
  for (int s = 0; s < G.nsegs; ++s) cnt[(size_t)s * n + i] = q == s ? 1 : 0;
}

// records [3 + nd + ni] doubles: position, the doubles, the ints
__global__ void k_mg_pack(int n, int nd, int ni, const double *__restrict__ xw, const double *__restrict__ fd, const int *__restrict__ fi,
                          const int *__restrict__ dest, const int *__restrict__ off, double *__restrict__ rec) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int q = dest[i];
  if (q < 0) return;
  const int w = 3 + nd + ni;
  double *r = rec + (size_t)off[(size_t)q * n + i] * w;
  for (int a = 0; a < 3; ++a) r[a] = xw[3 * (size_t)i + a];
  for (int k = 0; k < nd; ++k) r[3 + k] = fd[(size_t)i * nd + k];
  for (int k = 0; k < ni; ++k) r[3 + nd + k] = (double)fi[(size_t)i * ni + k];
}

__global__ void k_mg_unpack(int nnew, int nstay, int nd, int ni, const double *__restrict__ sbuf, const double *__restrict__ rbuf,
                            double *__restrict__ x, double *__restrict__ fd, int *__restrict__ fi) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nnew) return;
  const int w = 3 + nd + ni;
  const double *r = i < nstay ? sbuf + (size_t)i * w : rbuf + (size_t)(i - nstay) * w;
  for (int a = 0; a < 3; ++a) x[3 * (size_t)i + a] = r[a];
  for (int k = 0; k < nd; ++k) fd[(size_t)i * nd + k] = r[3 + k];
  for (int k = 0; k < ni; ++k) fi[(size_t)i * ni + k] = (int)r[3 + nd + k];
}

inline int migrate(isph_ctx *ctx, const isph_decomp *dc, int n, const double *x, int nd, const double *fd, int ni, const int *fi,
                   int on_device, isph_migrated &M) {
  hipStream_t st = ctx->stream;
  const bool dist = comm_active(ctx) && ctx->nranks > 1;
  DdHost D;
  MgGeom G;
  memset(&G, 0, sizeof(G));
  DevTmp<double> xin, fdin, xw, sbuf, rbuf, dfaces;
  DevTmp<int> fiin, dest, cnt, off, far;
  std::vector<int> count;   // per segment
  const int w = 3 + nd + ni;
  M.nd = nd; M.ni = ni;
  int nfar_out = 0;
  auto local = [&]() -> int {
    ISPH_CHECK(dd_setup(ctx, dc, 0.0, false, D));
    ISPH_REQUIRE(n >= 0 && n <= INT_MAX / 32, "nlocal out of range");
    ISPH_REQUIRE(nd >= 0 && ni >= 0 && nd + ni <= 1024, "isph_migrate: nd / ni out of range");
    G.dim = D.G.dim; G.me = D.G.me;
    G.nsegs = 1 + (int)D.peer.size();
    std::vector<double> hf;
    for (int a = 0; a < 3; ++a) {
      G.lo[a] = D.G.lo[a]; G.period[a] = D.G.period[a]; G.periodic[a] = D.G.periodic[a];
      G.pg[a] = D.pg[a]; G.c[a] = D.c[a];
      G.foff[a] = (int)hf.size();
      hf.insert(hf.end(), D.faces[a].begin(), D.faces[a].end());
    }
    for (int dz = -1; dz <= 1; ++dz)
      for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
          const int d[3] = {dx, dy, dz};
          int tc[3], q = 0;
          for (int a = 0; a < 3 && q >= 0; ++a) {
            tc[a] = D.c[a] + d[a];
            if (tc[a] < 0 || tc[a] >= D.pg[a]) {
              if (!D.G.periodic[a] || (D.pg[a] == 1 && d[a] != 0)) q = -1;
              else tc[a] = (tc[a] + D.pg[a]) % D.pg[a];
            }
          }
          if (q >= 0) {
            const int r = dd_rank_of(D.pg, tc);
            q = r == G.me ? 0 : 1 + (int)(std::lower_bound(D.peer.begin(), D.peer.end(), r) - D.peer.begin());
          }
          G.seg_of[(dz + 1) * 9 + (dy + 1) * 3 + dx + 1] = q;
        }
    count.assign((size_t)G.nsegs, 0);
    if (n == 0) return ISPH_SUCCESS;
    ISPH_REQUIRE(x && (fd || nd == 0) && (fi || ni == 0), "NULL argument");
    const double *dx = nullptr, *dfd = nullptr;
    const int *dfi = nullptr;
    ISPH_CHECK(dd_stage_in(ctx, x, (size_t)n * 3, on_device, xin, &dx));
    ISPH_CHECK(dd_stage_in(ctx, fd, (size_t)n * nd, on_device, fdin, &dfd));
    ISPH_CHECK(dd_stage_in(ctx, fi, (size_t)n * ni, on_device, fiin, &dfi));
    const size_t nc = (size_t)G.nsegs * (size_t)n + 1;
    ISPH_REQUIRE(nc < (size_t)INT_MAX, "too many particles");
    ISPH_CHECK(dfaces.reserve(hf.size()));
    ISPH_CHECK(xw.reserve((size_t)n * 3));
    ISPH_CHECK(dest.reserve((size_t)n));
    ISPH_CHECK(cnt.reserve(nc));
    ISPH_CHECK(off.reserve(nc));
    ISPH_CHECK(far.reserve(1));
    ISPH_CHECK(sbuf.reserve((size_t)n * w));
    ISPH_CHECK_HIP(hipMemcpyAsync(dfaces.p, hf.data(), sizeof(double) * hf.size(), hipMemcpyHostToDevice, st));
    ISPH_CHECK_HIP(hipMemsetAsync(far.p, 0, sizeof(int), st));
    ISPH_CHECK_HIP(hipMemsetAsync(cnt.p + (nc - 1), 0, sizeof(int), st));
    hipLaunchKernelGGL(k_mg_dest, dd_grid(n), dim3(kBlock), 0, st, n, G, (const double *)dfaces.p, dx, xw.p, dest.p, cnt.p, far.p);
    ISPH_CHECK(nl_exclusive_scan<int>(st, cnt.p, off.p, nc));
    hipLaunchKernelGGL(k_mg_pack, dd_grid(n), dim3(kBlock), 0, st, n, nd, ni, (const double *)xw.p, dfd, dfi, (const int *)dest.p,
                       (const int *)off.p, sbuf.p);
    DdAt A;
    A.m = G.nsegs + 1;
    for (int q = 0; q <= G.nsegs; ++q) A.at[q] = (int)((size_t)q * (size_t)n);
    int h[kDdSegs + 2], nfar = 0;
    ISPH_CHECK_HIP(hipMemcpyAsync(&nfar, far.p, sizeof(int), hipMemcpyDeviceToHost, st));
    ISPH_CHECK(dd_read_at(ctx, A, off.p, h));   // synchronises: the staged inputs may go
    for (int q = 0; q < G.nsegs; ++q) count[(size_t)q] = h[q + 1] - h[q];
    nfar_out = nfar;
    return ISPH_SUCCESS;
  };
  int rc = local();
  double nfar_all = (double)nfar_out;
  if (!comm_consensus(ctx, dist, "migrate", "migrate: the consensus all-reduce failed", &nfar_all, 1, rc)) return rc;
  if (nfar_all != 0.0) {
    char msg[160];
    snprintf(msg, sizeof(msg), "isph_migrate: a particle moved farther than one sub-box (%d on this rank)", nfar_out);
    return fail(msg, __FILE__, __LINE__);
  }
  std::vector<int> nsend(count.begin() + 1, count.end()), nrecv;
  ISPH_CHECK(dd_exchange_counts(ctx, D.peer, nsend, nrecv));
  isph_halo H;
  dd_make_halo(D.peer, nsend, nrecv, H);
  const int nstay = count[0];
  const long long nnew = (long long)nstay + H.nrecv;
  rc = nnew < (long long)INT_MAX / 32 ? ISPH_SUCCESS : fail("too many particles", __FILE__, __LINE__);
  if (rc == ISPH_SUCCESS) rc = rbuf.reserve((size_t)(H.nrecv > 0 ? H.nrecv : 1) * w);
  if (rc == ISPH_SUCCESS) rc = sbuf.reserve(1);
  if (rc == ISPH_SUCCESS) rc = M.x.reserve((size_t)(nnew > 0 ? nnew : 1) * 3);
  if (rc == ISPH_SUCCESS) rc = M.fd.reserve((size_t)(nnew > 0 ? nnew : 1) * (nd > 0 ? nd : 1));
  if (rc == ISPH_SUCCESS) rc = M.fi.reserve((size_t)(nnew > 0 ? nnew : 1) * (ni > 0 ? ni : 1));
  if (!comm_consensus(ctx, dist, "migrate", "migrate: the consensus all-reduce failed", nullptr, 0, rc)) return rc;
  ISPH_CHECK(comm_exchange(ctx, H, sbuf.p + (size_t)nstay * w, rbuf.p, w, false, st));
  if (nnew > 0)
    hipLaunchKernelGGL(k_mg_unpack, dd_grid(nnew), dim3(kBlock), 0, st, (int)nnew, nstay, nd, ni, (const double *)sbuf.p,
                       (const double *)rbuf.p, M.x.p, M.fd.p, M.fi.p);
  ISPH_CHECK_HIP(hipStreamSynchronize(st));
  ISPH_CHECK_HIP(hipGetLastError());
  M.nlocal = (int)nnew; M.nsent = H.nsend; M.nrecv = H.nrecv;
  return ISPH_SUCCESS;
}

}  // namespace isph

extern "C" {

int isph_nlist_build_dist(isph_ctx *ctx, const isph_decomp *dc, int nlocal, const double *x, double cut, int prune, int on_device,
                          isph_nlist **out) {
  using namespace isph;
  ISPH_REQUIRE(ctx && dc && out, "NULL argument");
  ISPH_REQUIRE(x || nlocal <= 0, "x is NULL");
  isph_nlist *L = new isph_nlist();
  const int rc = nlist_build_dist(ctx, dc, nlocal, x, cut, prune, on_device, *L);
  if (rc != ISPH_SUCCESS) {
    L->release();
    delete L;
    return rc;
  }
  *out = L;
  return ISPH_SUCCESS;
}

int isph_nlist_dist_info(const isph_nlist *nl, long long info[8]) {
  ISPH_REQUIRE(nl && info, "NULL argument");
  ISPH_REQUIRE(nl->dist, "isph_nlist_dist_info: the list was not built by isph_nlist_build_dist");
  info[0] = nl->nlocal; info[1] = nl->nghost; info[2] = nl->nnz; info[3] = nl->fits32;
  info[4] = nl->ncol; info[5] = nl->halo.npeers; info[6] = nl->halo.nsend; info[7] = nl->noffrank;
  return ISPH_SUCCESS;
}

int isph_nlist_dist_get(isph_ctx *ctx, const isph_nlist *nl, int *owner_rank, int *colmap, int *peers, int *send_ptr, int *send_idx,
                        int *recv_ptr, int on_device) {
  using namespace isph;
  ISPH_REQUIRE(ctx && nl, "NULL argument");
  ISPH_REQUIRE(nl->dist, "isph_nlist_dist_get: the list was not built by isph_nlist_build_dist");
  const size_t nall = (size_t)nl->nlocal + (size_t)nl->nghost, np = (size_t)nl->halo.npeers;
  ISPH_CHECK(nl_copy_out(ctx, owner_rank, (const int *)nl->orank.p, nall, on_device));
  ISPH_CHECK(nl_copy_out(ctx, colmap, (const int *)nl->colmap.p, nall, on_device));
  ISPH_CHECK(nl_copy_out(ctx, send_idx, (const int *)nl->halo.send_idx.p, (size_t)nl->halo.nsend, on_device));
  const hipMemcpyKind kind = on_device ? hipMemcpyHostToDevice : hipMemcpyHostToHost;
  const struct { int *dst; const int *src; size_t count; } small[3] = {
      {peers, nl->halo.peer.data(), np}, {send_ptr, nl->halo.send_ptr.data(), np + 1}, {recv_ptr, nl->halo.recv_ptr.data(), np + 1}};
  for (const auto &s : small) {
    if (!s.dst || s.count == 0) continue;
    ISPH_REQUIRE(on_device || !is_device_pointer(s.dst), "on_device = 0 but an output is device memory");
    ISPH_CHECK_HIP(hipMemcpyAsync(s.dst, s.src, sizeof(int) * s.count, kind, ctx->stream));
  }
  ISPH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  return ISPH_SUCCESS;
}

int isph_nlist_forward(isph_ctx *ctx, const isph_nlist *nl, int ncomp, double *a, int on_device) {
  ISPH_REQUIRE(ctx && nl, "NULL argument");
  return isph::nlist_forward<double>(ctx, nl, ncomp, a, on_device);
}

int isph_nlist_forward_int(isph_ctx *ctx, const isph_nlist *nl, int ncomp, int *a, int on_device) {
  ISPH_REQUIRE(ctx && nl, "NULL argument");
  return isph::nlist_forward<int>(ctx, nl, ncomp, a, on_device);
}

int isph_nlist_forward_multi(isph_ctx *ctx, const isph_nlist *nl, int narrays, const isph_fwd_array *arr, int on_device) {
  ISPH_REQUIRE(ctx && nl, "NULL argument");
  return isph::nlist_forward_multi(ctx, nl, narrays, arr, on_device, /*agree=*/true);
}

int isph_migrate(isph_ctx *ctx, const isph_decomp *dc, int nlocal, const double *x, int nd, const double *fd, int ni, const int *fi,
                 int on_device, isph_migrated **out) {
  using namespace isph;
  ISPH_REQUIRE(ctx && dc && out, "NULL argument");
  isph_migrated *M = new isph_migrated();
  const int rc = migrate(ctx, dc, nlocal, x, nd, fd, ni, fi, on_device, *M);
  if (rc != ISPH_SUCCESS) {
    M->release();
    delete M;
    return rc;
  }
  *out = M;
  return ISPH_SUCCESS;
}

int isph_migrated_info(const isph_migrated *mg, long long info[3]) {
  ISPH_REQUIRE(mg && info, "NULL argument");
  info[0] = mg->nlocal; info[1] = mg->nsent; info[2] = mg->nrecv;
  return ISPH_SUCCESS;
}

int isph_migrated_get(isph_ctx *ctx, const isph_migrated *mg, double *x, double *fd, int *fi, int on_device) {
  using namespace isph;
  ISPH_REQUIRE(ctx && mg, "NULL argument");
  const size_t n = (size_t)mg->nlocal;
  ISPH_CHECK(nl_copy_out(ctx, x, (const double *)mg->x.p, n * 3, on_device));
  ISPH_CHECK(nl_copy_out(ctx, fd, (const double *)mg->fd.p, n * (size_t)mg->nd, on_device));
  ISPH_CHECK(nl_copy_out(ctx, fi, (const int *)mg->fi.p, n * (size_t)mg->ni, on_device));
  ISPH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  return ISPH_SUCCESS;
}

int isph_migrated_destroy(isph_ctx *ctx, isph_migrated *mg) {
  (void)ctx;
  if (!mg) return ISPH_SUCCESS;
  mg->release();
  delete mg;
  return ISPH_SUCCESS;
}

}  // extern "C"
