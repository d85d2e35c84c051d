// step_ops.hpp -- the glue of a time step that is no neighbour sweep: the forward comm of periodic images on one rank,
// computeZeroMeanPressure, and the two observables the reference's scripts record (compute isph/status, fix isph/tgv).
// Included by isph_capi.hip; every entry point is usable on its own.  The last three have a collective form over the
// ranks of a communicator (isph_*_dist, at the end of the namespace).
//
// Reductions follow the discipline of the solvers' multi-dot (krylov.hpp): a grid that depends on n alone, every block
// sums a fixed set of rows in a fixed order into its own slot, one block per quantity then sums the slots in a fixed
// order.  No floating-point atomics: the bits do not change from run to run.
#pragma once
#include <cmath>

#include "amg.hpp"  // wave_max_f64
#include "assemble.hpp"
#include "comm.hpp"
#include "core.hpp"
#include "operators.hpp"  // InOut

namespace isph {

constexpr int kKindSolid = 12;  // pair_isph.h:113-124

inline int step_red_grid(long long n) {
  long long g = (n + kBlock - 1) / kBlock;
  if (g < 1) g = 1;
  return (int)(g > kMaxRedBlocks ? kMaxRedBlocks : g);
}

// the block's NS sums (and one maximum when WITH_MAX) into partial[k * gridDim.x + blockIdx.x]; the maximum is quantity NS
template <int NS, bool WITH_MAX>
__device__ __forceinline__ void block_partials(const double (&acc)[NS], double vmax, double *__restrict__ partial) {
  __shared__ double sred[NS + 1][4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    const double s = wave_sum(acc[k]);
    if (lane == 0) sred[k][wave] = s;
  }
  if (WITH_MAX) {
    const double m = wave_max_f64(vmax);
    if (lane == 0) sred[NS][wave] = m;
  }
  __syncthreads();
  if (threadIdx.x < NS)
    partial[(long long)threadIdx.x * gridDim.x + blockIdx.x] =
        (sred[threadIdx.x][0] + sred[threadIdx.x][1]) + (sred[threadIdx.x][2] + sred[threadIdx.x][3]);
  if (WITH_MAX && threadIdx.x == NS)
    partial[(long long)NS * gridDim.x + blockIdx.x] = fmax(fmax(sred[NS][0], sred[NS][1]), fmax(sred[NS][2], sred[NS][3]));
}

// second stage: out[k] = sum (k == kmax: max) over b of partial[k * nblk + b]; one block per k, fixed order
__global__ __launch_bounds__(kBlock) void k_step_reduce(int nblk, int kmax, const double *__restrict__ partial,
                                                        double *__restrict__ out) {
  __shared__ double sw[4];
  const int k = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const double *__restrict__ p = partial + (long long)k * nblk;
  const bool is_max = k == kmax;
  double a = 0.0;
  for (int b = threadIdx.x; b < nblk; b += kBlock) a = is_max ? fmax(a, p[b]) : a + p[b];
  a = is_max ? wave_max_f64(a) : wave_sum(a);
  if (lane == 0) sw[wave] = a;
  __syncthreads();
  if (threadIdx.x == 0) out[k] = is_max ? fmax(fmax(sw[0], sw[1]), fmax(sw[2], sw[3])) : (sw[0] + sw[1]) + (sw[2] + sw[3]);
}

__device__ __forceinline__ int kind_of(const int *__restrict__ type, const int *__restrict__ kind, int ntypes, long long i) {
  const int t = type[i];
  return (t >= 0 && t <= ntypes) ? kind[t] : 0;
}

// ---- forward comm of periodic images -------------------------------------------------------------------------------

// one thread per component of a ghost row: consecutive threads read consecutive components of the owner's row
__global__ __launch_bounds__(kBlock) void k_ghost_fill(int nlocal, long long nelem, int ncomp, const int *__restrict__ owner,
                                                       double *__restrict__ a, int *__restrict__ flag) {
  const long long e = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (e >= nelem) return;
  const long long g = e / ncomp;
  const int c = (int)(e - g * ncomp);
  const int o = owner[nlocal + g];
  if (o < 0 || o >= nlocal) {
    if (flag) *flag = 1;
    return;
  }
  a[((long long)nlocal + g) * ncomp + c] = a[(long long)o * ncomp + c];
}

// device operands.  check: the owners are validated -- one flag is copied back; without it (a map that has been validated
// before) nothing is read back and a row with a bad owner is skipped
inline int ghost_fill_device(isph_ctx *ctx, int nlocal, int nall, const int *d_owner, int ncomp, double *d_a, bool check = true) {
  const long long nelem = (long long)(nall - nlocal) * ncomp;
  if (nelem == 0) return ISPH_SUCCESS;
  const long long blocks = (nelem + kBlock - 1) / kBlock;
  ISPH_REQUIRE(blocks < (1ll << 31), "ghost fill: too many elements");
  if (!check) {
    hipLaunchKernelGGL(k_ghost_fill, dim3((unsigned)blocks), dim3(kBlock), 0, ctx->stream, nlocal, nelem, ncomp, d_owner, d_a,
                       (int *)nullptr);
    ISPH_CHECK_HIP(hipGetLastError());
    return ISPH_SUCCESS;
  }
  DevTmp<int> flag;
  ISPH_CHECK(flag.reserve(1));
  ISPH_CHECK_HIP(hipMemsetAsync(flag.p, 0, sizeof(int), ctx->stream));
  hipLaunchKernelGGL(k_ghost_fill, dim3((unsigned)blocks), dim3(kBlock), 0, ctx->stream, nlocal, nelem, ncomp, d_owner, d_a, flag.p);
  int bad = 0;
  ISPH_CHECK_HIP(hipMemcpyAsync(&bad, flag.p, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  ISPH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  ISPH_CHECK_HIP(hipGetLastError());
  ISPH_REQUIRE(!bad, "isph_ghost_fill: owner of a ghost row is not an owned row (owner[i] outside [0, nlocal))");
  return ISPH_SUCCESS;
}

// ---- computeZeroMeanPressure -----------------------------------------------------------------------------------------

// owned rows: Solid -> 0 (whatever it held), the others enter the sum and the count
__global__ __launch_bounds__(kBlock) void k_zero_mean_sum(int nlocal, int ntypes, const int *__restrict__ type,
                                                          const int *__restrict__ kind, double *__restrict__ f,
                                                          double *__restrict__ partial) {
  double acc[2] = {0.0, 0.0};
  const long long stride = (long long)gridDim.x * kBlock;
  for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < nlocal; i += stride) {
    if (kind_of(type, kind, ntypes, i) == kKindSolid) f[i] = 0.0;
    else { acc[0] += f[i]; acc[1] += 1.0; }
  }
  block_partials<2, false>(acc, 0.0, partial);
}

// scal = {sum, count}; mean = sum / count, 0 for an empty set; all nall rows that are not Solid lose the mean
__global__ __launch_bounds__(kBlock) void k_zero_mean_subtract(int nall, int ntypes, const int *__restrict__ type,
                                                               const int *__restrict__ kind, const double *__restrict__ scal,
                                                               double *__restrict__ f) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= nall || scal[1] == 0.0) return;
  const double mean = scal[0] / scal[1];
  if (kind_of(type, kind, ntypes, i) != kKindSolid) f[i] -= mean;
}

// device operands; d_kind [ntypes + 1] on the device
inline int zero_mean_device(isph_ctx *ctx, int nlocal, int nall, const int *d_type, const int *d_kind, int ntypes, double *d_f,
                            int update, double *mean_out) {
  DevTmp<double> partial, scal;
  const int g = step_red_grid(nlocal);
  ISPH_CHECK(partial.reserve((size_t)2 * g));
  ISPH_CHECK(scal.reserve(2));
  hipLaunchKernelGGL(k_zero_mean_sum, dim3(g), dim3(kBlock), 0, ctx->stream, nlocal, ntypes, d_type, d_kind, d_f, partial.p);
  hipLaunchKernelGGL(k_step_reduce, dim3(2), dim3(kBlock), 0, ctx->stream, g, -1, (const double *)partial.p, scal.p);
  if (update && nall > 0)
    hipLaunchKernelGGL(k_zero_mean_subtract, dim3((nall + kBlock - 1) / kBlock), dim3(kBlock), 0, ctx->stream, nall, ntypes,
                       d_type, d_kind, (const double *)scal.p, d_f);
  ISPH_CHECK_HIP(hipGetLastError());
  if (mean_out) {
    double h[2] = {0.0, 0.0};
    ISPH_CHECK_HIP(hipMemcpyAsync(h, scal.p, 2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    ISPH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    *mean_out = h[1] == 0.0 ? 0.0 : h[0] / h[1];
  }
  return ISPH_SUCCESS;
}

// ---- compute isph/status ---------------------------------------------------------------------------------------------

struct StatusArgs {
  int nlocal, type_mask, with_max;
  double c[3], rsq_max;  // r <= radius as a test on r^2: rsq_max is the largest double whose rounded root is <= radius
};

// every product and sum rounded on its own: the terms are those of the reference's loop.  The contraction is switched off
// for the statements of this kernel (HIP contracts a * b + c by default, and its __dmul_rn / __dadd_rn are plain
// operators that contract as well)
__global__ __launch_bounds__(kBlock) void k_status(StatusArgs s, const double *__restrict__ x, const int *__restrict__ type,
                                                   const double *__restrict__ vfrac, const double *__restrict__ v,
                                                   const double *__restrict__ rho, double *__restrict__ partial) {
#pragma clang fp contract(off)
  double acc[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double vmax = 0.0;
  const long long stride = (long long)gridDim.x * kBlock;
  for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < s.nlocal; i += stride) {
    const int sh = type[i] - 1;
    if (sh < 0 || sh > 31 || !((unsigned)s.type_mask & (1u << sh))) continue;
    const double vx = v[3 * i], vy = v[3 * i + 1], vz = v[3 * i + 2];
    const double vmagsq = (vx * vx + vy * vy) + vz * vz;
    const double vf = vfrac[i];
    const double mass = rho[i] * vf;
    acc[0] += 1.0;
    acc[1] += vx; acc[2] += vy; acc[3] += vz;
    acc[4] += vf;
    acc[5] += mass;
    const double ke = (0.5 * mass) * vmagsq;
    acc[6] += ke;
    if (s.with_max) {
      const double x0 = x[3 * i] - s.c[0], x1 = x[3 * i + 1] - s.c[1], x2 = x[3 * i + 2] - s.c[2];
      const double rsq = (x0 * x0 + x1 * x1) + x2 * x2;
      if (rsq <= s.rsq_max) vmax = fmax(vmax, vmagsq);
    }
  }
  block_partials<7, true>(acc, vmax, partial);
}

// ---- fix isph/tgv ------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kBlock) void k_tgv_pressure_sum(int nlocal, const double *__restrict__ p, double *__restrict__ partial) {
  double acc[1] = {0.0};
  const long long stride = (long long)gridDim.x * kBlock;
  for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < nlocal; i += stride) acc[0] += p[i];
  block_partials<1, false>(acc, 0.0, partial);
}

// the four sums of this rank's rows with the pressure mean pavg_diff removed; the exact pressure has mean 0
// (fix_isph_tgv.cpp:77)
__device__ __forceinline__ void tgv_error_sums(int nlocal, double t, double umax, double pavg_diff, const double *__restrict__ x,
                                               const double *__restrict__ vnp1, const double *__restrict__ p,
                                               const double *__restrict__ rho, const double *__restrict__ nu,
                                               double *__restrict__ partial) {
  double acc[4] = {0.0, 0.0, 0.0, 0.0};  // errorp, normp, erroru, normu
  const long long stride = (long long)gridDim.x * kBlock;
  for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < nlocal; i += stride) {
    const double x0 = x[3 * i], x1 = x[3 * i + 1];
    const double pe = 0.25 * rho[i] * (cos(2.0 * x0) + cos(2.0 * x1)) * umax * umax * exp(-4.0 * nu[i] * t);
    const double dec = umax * exp(-2.0 * nu[i] * t);
    const double u0 = dec * sin(x0) * cos(x1), u1 = -dec * cos(x0) * sin(x1);
    const double ep = p[i] - pe - pavg_diff;
    const double e0 = vnp1[3 * i] - u0, e1 = vnp1[3 * i + 1] - u1, e2 = vnp1[3 * i + 2];
    acc[0] += ep * ep;
    acc[1] += pe * pe;
    acc[2] += e0 * e0 + e1 * e1 + e2 * e2;
    acc[3] += u0 * u0 + u1 * u1;
  }
  block_partials<4, false>(acc, 0.0, partial);
}

// psum[0] = sum of p over the owned rows (on the device)
__global__ __launch_bounds__(kBlock) void k_tgv_error(int nlocal, double t, double umax, const double *__restrict__ psum,
                                                      const double *__restrict__ x, const double *__restrict__ vnp1,
                                                      const double *__restrict__ p, const double *__restrict__ rho,
                                                      const double *__restrict__ nu, double *__restrict__ partial) {
  tgv_error_sums(nlocal, t, umax, nlocal > 0 ? psum[0] / (double)nlocal : 0.0, x, vnp1, p, rho, nu, partial);
}

// device operands; out[4] on the host
inline int tgv_error_device(isph_ctx *ctx, int nlocal, const double *d_x, const double *d_vnp1, const double *d_p,
                            const double *d_rho, const double *d_nu, double t, double umax, double out[4]) {
  DevTmp<double> partial, scal;
  const int g = step_red_grid(nlocal);
  ISPH_CHECK(partial.reserve((size_t)4 * g));
  ISPH_CHECK(scal.reserve(5));
  hipLaunchKernelGGL(k_tgv_pressure_sum, dim3(g), dim3(kBlock), 0, ctx->stream, nlocal, d_p, partial.p);
  hipLaunchKernelGGL(k_step_reduce, dim3(1), dim3(kBlock), 0, ctx->stream, g, -1, (const double *)partial.p, scal.p + 4);
  hipLaunchKernelGGL(k_tgv_error, dim3(g), dim3(kBlock), 0, ctx->stream, nlocal, t, umax, (const double *)(scal.p + 4), d_x,
                     d_vnp1, d_p, d_rho, d_nu, partial.p);
  hipLaunchKernelGGL(k_step_reduce, dim3(4), dim3(kBlock), 0, ctx->stream, g, -1, (const double *)partial.p, scal.p);
  double h[4];
  ISPH_CHECK_HIP(hipMemcpyAsync(h, scal.p, 4 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  ISPH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  ISPH_CHECK_HIP(hipGetLastError());
  for (int k = 0; k < 4; ++k) out[k] = nlocal > 0 ? std::sqrt(h[k] / (double)nlocal) : 0.0;
  return ISPH_SUCCESS;
}

// the arguments of k_status.  The reference tests sqrt(r^2) <= radius and keeps max sqrt(|v|^2).  The correctly rounded
// root is monotone, so the first is a threshold on r^2 and the second is the root of the maximum: both roots are taken on
// the host, exactly.
inline StatusArgs status_args(int nlocal, int type_mask, const double centre[3], double radius) {
  StatusArgs s;
  s.nlocal = nlocal; s.type_mask = type_mask;
  s.with_max = radius > 0.0;
  s.rsq_max = radius * radius;
  if (s.with_max && std::isfinite(s.rsq_max)) {
    while (std::sqrt(s.rsq_max) > radius) s.rsq_max = std::nextafter(s.rsq_max, 0.0);
    while (std::isfinite(s.rsq_max) && std::sqrt(std::nextafter(s.rsq_max, INFINITY)) <= radius)
      s.rsq_max = std::nextafter(s.rsq_max, INFINITY);
  }
  for (int k = 0; k < 3; ++k) s.c[k] = centre[k];
  return s;
}

// device operands; out[8] on the host
inline int status_device(isph_ctx *ctx, int nlocal, int type_mask, const double *d_x, const int *d_type, const double *d_vfrac,
                         const double *d_v, const double *d_rho, const double centre[3], double radius, double out[8]) {
  DevTmp<double> partial, scal;
  const int g = step_red_grid(nlocal);
  ISPH_CHECK(partial.reserve((size_t)8 * g));
  ISPH_CHECK(scal.reserve(8));
  const StatusArgs s = status_args(nlocal, type_mask, centre, radius);
  hipLaunchKernelGGL(k_status, dim3(g), dim3(kBlock), 0, ctx->stream, s, d_x, d_type, d_vfrac, d_v, d_rho, partial.p);
  hipLaunchKernelGGL(k_step_reduce, dim3(8), dim3(kBlock), 0, ctx->stream, g, 7, (const double *)partial.p, scal.p);
  ISPH_CHECK_HIP(hipMemcpyAsync(out, scal.p, 8 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  ISPH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  ISPH_CHECK_HIP(hipGetLastError());
  out[7] = std::sqrt(out[7]);
  return ISPH_SUCCESS;
}

inline int step_one_rank(const isph_ctx *ctx, const char *msg) {
  ISPH_REQUIRE(ctx->nranks == 1 && !ctx->comm && !ctx->host_tr.allreduce, msg);
  return ISPH_SUCCESS;
}

// ---- the same three over the ranks of a communicator -----------------------------------------------------------------
// Per rank the two-stage reduction above; the second stage writes the rank's sums into ITS slot of an [nranks][nq] vector
// and zeros into the others, one sum all-reduce adds the vectors (adding zeros is exact, so every slot arrives with the
// bits its rank computed, whatever order the transport adds in), and k_step_slot_combine adds the slots in rank order.
// The maximum goes through a max all-reduce.  The bits of a result are the same on every rank, from run to run and from
// transport to transport.  Without a communicator the one-rank forms above are called: their bits.

inline bool step_dist(const isph_ctx *ctx) { return comm_active(ctx); }
inline int step_rank(const isph_ctx *ctx) { return comm_active(ctx) ? ctx->rank : 0; }
inline int step_nranks(const isph_ctx *ctx) { return comm_active(ctx) ? ctx->nranks : 1; }

// second stage on a rank of several: block k sums partial[k * nblk + .] in the fixed order of k_step_reduce and writes
// slots[r * nq + k] for every rank r -- the sum for r == rank, 0 for the others; quantity kmax is a maximum and goes to
// maxout[0].  extra (k == kextra): a number the host knows (a row count) takes the place of the sum.
__global__ __launch_bounds__(kBlock) void k_step_reduce_slots(int nblk, int kmax, int nranks, int rank, int nq, int kextra,
                                                              double extra, const double *__restrict__ partial,
                                                              double *__restrict__ slots, double *__restrict__ maxout) {
  __shared__ double sw[4];
  __shared__ double total;
  const int k = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const bool is_max = k == kmax;
  double a = 0.0;
  if (k != kextra) {
    const double *__restrict__ p = partial + (long long)k * nblk;
    for (int b = threadIdx.x; b < nblk; b += kBlock) a = is_max ? fmax(a, p[b]) : a + p[b];
  }
  a = is_max ? wave_max_f64(a) : wave_sum(a);
  if (lane == 0) sw[wave] = a;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double t = is_max ? fmax(fmax(sw[0], sw[1]), fmax(sw[2], sw[3])) : (sw[0] + sw[1]) + (sw[2] + sw[3]);
    total = k == kextra ? extra : t;
    if (is_max) maxout[0] = t;
  }
  __syncthreads();
  if (is_max) return;
  for (int r = threadIdx.x; r < nranks; r += kBlock) slots[(long long)r * nq + k] = r == rank ? total : 0.0;
}

// out[k] = slots[0][k] + slots[1][k] + ... in rank order: one thread per quantity
__global__ __launch_bounds__(kBlock) void k_step_slot_combine(int nranks, int nq, const double *__restrict__ slots,
                                                              double *__restrict__ out) {
  const int k = blockIdx.x * kBlock + threadIdx.x;
  if (k >= nq) return;
  double a = 0.0;
  for (int r = 0; r < nranks; ++r) a += slots[(long long)r * nq + k];
  out[k] = a;
}

// partial [nq x g] of this rank -> out[0 .. nq) summed over the ranks (on the device); quantity kmax, when >= 0, is not
// part of nq: its maximum over the ranks lands in out[nq]
inline int step_sum_ranks(isph_ctx *ctx, int g, int nq, int kmax, int kextra, double extra, const double *partial, double *out) {
  const int nr = step_nranks(ctx);
  DevTmp<double> slots;
  ISPH_CHECK(slots.reserve((size_t)nr * nq));
  hipLaunchKernelGGL(k_step_reduce_slots, dim3(nq + (kmax >= 0 ? 1 : 0)), dim3(kBlock), 0, ctx->stream, g, kmax, nr, step_rank(ctx),
                     nq, kextra, extra, partial, slots.p, out + nq);
  ISPH_CHECK_HIP(hipGetLastError());
  ISPH_CHECK(comm_allreduce(ctx, slots.p, nr * nq, /*sum*/ 0, ctx->stream));
  if (kmax >= 0) ISPH_CHECK(comm_allreduce(ctx, out + nq, 1, /*max*/ 1, ctx->stream));
  hipLaunchKernelGGL(k_step_slot_combine, dim3((nq + kBlock - 1) / kBlock), dim3(kBlock), 0, ctx->stream, nr, nq,
                     (const double *)slots.p, out);
  ISPH_CHECK_HIP(hipGetLastError());
  // the slots go back to the pool when this returns: the combine must have read them (the pool parks a block until the
  // device has been synchronised, so the launch above is safe)
  return ISPH_SUCCESS;
}

// zero_mean_device over all ranks: one sum all-reduce
inline int zero_mean_dist_device(isph_ctx *ctx, int nlocal, int nall, const int *d_type, const int *d_kind, int ntypes, double *d_f,
                                 int update, double *mean_out) {
  if (!step_dist(ctx)) return zero_mean_device(ctx, nlocal, nall, d_type, d_kind, ntypes, d_f, update, mean_out);
  DevTmp<double> partial, scal;
  const int g = step_red_grid(nlocal);
  ISPH_CHECK(partial.reserve((size_t)2 * g));
  ISPH_CHECK(scal.reserve(2));
  hipLaunchKernelGGL(k_zero_mean_sum, dim3(g), dim3(kBlock), 0, ctx->stream, nlocal, ntypes, d_type, d_kind, d_f, partial.p);
  ISPH_CHECK(step_sum_ranks(ctx, g, 2, -1, -1, 0.0, partial.p, scal.p));
  if (update && nall > 0)
    hipLaunchKernelGGL(k_zero_mean_subtract, dim3((nall + kBlock - 1) / kBlock), dim3(kBlock), 0, ctx->stream, nall, ntypes,
                       d_type, d_kind, (const double *)scal.p, d_f);
  ISPH_CHECK_HIP(hipGetLastError());
  if (mean_out) {
    double h[2] = {0.0, 0.0};
    ISPH_CHECK_HIP(hipMemcpyAsync(h, scal.p, 2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    ISPH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    *mean_out = h[1] == 0.0 ? 0.0 : h[0] / h[1];
  }
  return ISPH_SUCCESS;
}

// psum = {sum of p, number of rows} over the owned rows of ALL ranks
__global__ __launch_bounds__(kBlock) void k_tgv_error_dist(int nlocal, double t, double umax, const double *__restrict__ psum,
                                                           const double *__restrict__ x, const double *__restrict__ vnp1,
                                                           const double *__restrict__ p, const double *__restrict__ rho,
                                                           const double *__restrict__ nu, double *__restrict__ partial) {
  tgv_error_sums(nlocal, t, umax, psum[1] > 0.0 ? psum[0] / psum[1] : 0.0, x, vnp1, p, rho, nu, partial);
}

// tgv_error_device over all ranks: two sum all-reduces (the pressure mean and the row count, then the four sums)
inline int tgv_error_dist_device(isph_ctx *ctx, int nlocal, const double *d_x, const double *d_vnp1, const double *d_p,
                                 const double *d_rho, const double *d_nu, double t, double umax, double out[4]) {
  if (!step_dist(ctx)) return tgv_error_device(ctx, nlocal, d_x, d_vnp1, d_p, d_rho, d_nu, t, umax, out);
  DevTmp<double> partial, scal;
  const int g = step_red_grid(nlocal);
  ISPH_CHECK(partial.reserve((size_t)4 * g));
  ISPH_CHECK(scal.reserve(6));
  hipLaunchKernelGGL(k_tgv_pressure_sum, dim3(g), dim3(kBlock), 0, ctx->stream, nlocal, d_p, partial.p);
  ISPH_CHECK(step_sum_ranks(ctx, g, 2, -1, /*kextra=*/1, (double)nlocal, partial.p, scal.p + 4));
  hipLaunchKernelGGL(k_tgv_error_dist, dim3(g), dim3(kBlock), 0, ctx->stream, nlocal, t, umax, (const double *)(scal.p + 4), d_x,
                     d_vnp1, d_p, d_rho, d_nu, partial.p);
  ISPH_CHECK(step_sum_ranks(ctx, g, 4, -1, -1, 0.0, partial.p, scal.p));
  double h[6];
  ISPH_CHECK_HIP(hipMemcpyAsync(h, scal.p, 6 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  ISPH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  ISPH_CHECK_HIP(hipGetLastError());
  for (int k = 0; k < 4; ++k) out[k] = h[5] > 0.0 ? std::sqrt(h[k] / h[5]) : 0.0;
  return ISPH_SUCCESS;
}

// status_device over all ranks: one sum all-reduce of the seven sums, one max all-reduce
inline int status_dist_device(isph_ctx *ctx, int nlocal, int type_mask, const double *d_x, const int *d_type, const double *d_vfrac,
                              const double *d_v, const double *d_rho, const double centre[3], double radius, double out[8]) {
  if (!step_dist(ctx)) return status_device(ctx, nlocal, type_mask, d_x, d_type, d_vfrac, d_v, d_rho, centre, radius, out);
  DevTmp<double> partial, scal;
  const int g = step_red_grid(nlocal);
  ISPH_CHECK(partial.reserve((size_t)8 * g));
  ISPH_CHECK(scal.reserve(8));
  const StatusArgs s = status_args(nlocal, type_mask, centre, radius);
  hipLaunchKernelGGL(k_status, dim3(g), dim3(kBlock), 0, ctx->stream, s, d_x, d_type, d_vfrac, d_v, d_rho, partial.p);
  ISPH_CHECK(step_sum_ranks(ctx, g, 7, /*kmax=*/7, -1, 0.0, partial.p, scal.p));
  ISPH_CHECK_HIP(hipMemcpyAsync(out, scal.p, 8 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  ISPH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  ISPH_CHECK_HIP(hipGetLastError());
  out[7] = std::sqrt(out[7]);
  return ISPH_SUCCESS;
}

// the argument checks of a collective primitive are made by every rank before the first all-reduce: a rank whose
// arguments are refused fails the others with it
inline int step_agree(isph_ctx *ctx, const char *who, int rc) {
  const bool dist = comm_active(ctx) && ctx->nranks > 1;
  (void)comm_consensus(ctx, dist, who, "the consensus all-reduce failed", nullptr, 0, rc);
  return rc;
}

}  // namespace isph

extern "C" {

int isph_ghost_fill(isph_ctx *ctx, int nlocal, int nall, const int *owner, int ncomp, double *a, int on_device) {
  using namespace isph;
  ISPH_REQUIRE(ctx, "NULL argument");
  ISPH_CHECK(step_one_rank(ctx, "isph_ghost_fill: a context with a communicator is not supported (one rank only)"));
  ISPH_REQUIRE(nlocal >= 0 && nall >= nlocal && ncomp >= 1, "isph_ghost_fill: need 0 <= nlocal <= nall and ncomp >= 1");
  if (nall == nlocal) return ISPH_SUCCESS;
  ISPH_REQUIRE(owner && a, "NULL argument");
  DevTmp<int> sown;
  const int *down = nullptr;
  InOut ia;
  ISPH_CHECK(stage(ctx, owner, (size_t)nall, on_device, sown, &down));
  ISPH_CHECK(ia.open(ctx, a, (size_t)nall * ncomp, on_device));
  ISPH_CHECK(ghost_fill_device(ctx, nlocal, nall, down, ncomp, ia.dev));
  ISPH_CHECK(ia.close(ctx));
  ISPH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  return ISPH_SUCCESS;
}

int isph_zero_mean_pressure(isph_ctx *ctx, int nlocal, int nall, const int *type, const int *kind, int ntypes, double *f,
                            int update, double *mean_out, int on_device) {
  using namespace isph;
  ISPH_REQUIRE(ctx && type && kind && f, "NULL argument");
  ISPH_CHECK(step_one_rank(ctx, "isph_zero_mean_pressure: a context with a communicator is not supported (one rank only)"));
  ISPH_REQUIRE(nlocal >= 0 && nall >= nlocal && ntypes >= 0, "isph_zero_mean_pressure: need 0 <= nlocal <= nall, ntypes >= 0");
  DevTmp<int> stype, skind;
  const int *dtype = nullptr, *dkind = nullptr;
  InOut fi;
  ISPH_CHECK(stage(ctx, type, (size_t)nall, on_device, stype, &dtype));
  ISPH_CHECK(stage(ctx, kind, (size_t)ntypes + 1, 0, skind, &dkind));
  ISPH_CHECK(fi.open(ctx, f, (size_t)nall, on_device));
  ISPH_CHECK(zero_mean_device(ctx, nlocal, nall, dtype, dkind, ntypes, fi.dev, update, mean_out));
  ISPH_CHECK(fi.close(ctx));
  // the staged kind table is pageable host memory of the caller: the copy must have been consumed before returning
  ISPH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  return ISPH_SUCCESS;
}

int isph_status(isph_ctx *ctx, const isph_particles *P, int type_mask, const double *v, const double *rho,
                const double centre[3], double radius, double out[8], int on_device) {
  using namespace isph;
  ISPH_REQUIRE(ctx && P && v && rho && centre && out, "NULL argument");
  ISPH_CHECK(step_one_rank(ctx, "isph_status: a context with a communicator is not supported (one rank only)"));
  ISPH_REQUIRE(P->x && P->type && P->nlocal >= 0, "isph_status: x and type are needed");
  ISPH_REQUIRE(P->vfrac, "isph_status: P->vfrac is needed");
  const size_t n = (size_t)P->nlocal;
  DevTmp<double> sx, svf, sv, srho;
  DevTmp<int> stype;
  const double *dx = nullptr, *dvf = nullptr, *dv = nullptr, *drho = nullptr;
  const int *dtype = nullptr;
  ISPH_CHECK(stage(ctx, P->x, 3 * n, on_device, sx, &dx));
  ISPH_CHECK(stage(ctx, P->type, n, on_device, stype, &dtype));
  ISPH_CHECK(stage(ctx, P->vfrac, n, on_device, svf, &dvf));
  ISPH_CHECK(stage(ctx, v, 3 * n, on_device, sv, &dv));
  ISPH_CHECK(stage(ctx, rho, n, on_device, srho, &drho));
  return status_device(ctx, P->nlocal, type_mask, dx, dtype, dvf, dv, drho, centre, radius, out);
}

int isph_tgv_error(isph_ctx *ctx, int nlocal, int dim, const double *x, const double *vnp1, const double *p,
                   const double *rho, const double *nu, double t, double umax, double out[4], int on_device) {
  using namespace isph;
  ISPH_REQUIRE(ctx && x && vnp1 && p && rho && nu && out, "NULL argument");
  ISPH_CHECK(step_one_rank(ctx, "isph_tgv_error: a context with a communicator is not supported (one rank only)"));
  ISPH_REQUIRE(nlocal >= 0 && (dim == 2 || dim == 3), "isph_tgv_error: need nlocal >= 0 and dim 2 or 3");
  const size_t n = (size_t)nlocal;
  DevTmp<double> sx, sv, sp, srho, snu;
  const double *dx = nullptr, *dv = nullptr, *dp = nullptr, *drho = nullptr, *dnu = nullptr;
  ISPH_CHECK(stage(ctx, x, 3 * n, on_device, sx, &dx));
  ISPH_CHECK(stage(ctx, vnp1, 3 * n, on_device, sv, &dv));
  ISPH_CHECK(stage(ctx, p, n, on_device, sp, &dp));
  ISPH_CHECK(stage(ctx, rho, n, on_device, srho, &drho));
  ISPH_CHECK(stage(ctx, nu, n, on_device, snu, &dnu));
  return tgv_error_device(ctx, nlocal, dx, dv, dp, drho, dnu, t, umax, out);
}

int isph_zero_mean_pressure_dist(isph_ctx *ctx, int nlocal, int nall, const int *type, const int *kind, int ntypes, double *f,
                                 int update, double *mean_out, int on_device) {
  using namespace isph;
  ISPH_REQUIRE(ctx, "NULL argument");
  DevTmp<int> stype, skind;
  const int *dtype = nullptr, *dkind = nullptr;
  InOut fi;
  auto local = [&]() -> int {
    ISPH_REQUIRE(kind && (nall == 0 || (type && f)), "NULL argument");
    ISPH_REQUIRE(nlocal >= 0 && nall >= nlocal && ntypes >= 0, "isph_zero_mean_pressure_dist: need 0 <= nlocal <= nall, ntypes >= 0");
    ISPH_CHECK(stage(ctx, type, (size_t)nall, on_device, stype, &dtype));
    ISPH_CHECK(stage(ctx, kind, (size_t)ntypes + 1, 0, skind, &dkind));
    if (nall > 0) ISPH_CHECK(fi.open(ctx, f, (size_t)nall, on_device));
    return ISPH_SUCCESS;
  };
  ISPH_CHECK(step_agree(ctx, "isph_zero_mean_pressure_dist", local()));
  ISPH_CHECK(zero_mean_dist_device(ctx, nlocal, nall, dtype, dkind, ntypes, fi.dev, update, mean_out));
  if (nall > 0) ISPH_CHECK(fi.close(ctx));
  ISPH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  return ISPH_SUCCESS;
}

int isph_status_dist(isph_ctx *ctx, const isph_particles *P, int type_mask, const double *v, const double *rho,
                     const double centre[3], double radius, double out[8], int on_device) {
  using namespace isph;
  ISPH_REQUIRE(ctx && P && centre && out, "NULL argument");
  DevTmp<double> sx, svf, sv, srho;
  DevTmp<int> stype;
  const double *dx = nullptr, *dvf = nullptr, *dv = nullptr, *drho = nullptr;
  const int *dtype = nullptr;
  auto local = [&]() -> int {
    ISPH_REQUIRE(P->nlocal >= 0, "isph_status_dist: nlocal must not be negative");
    const size_t n = (size_t)P->nlocal;
    ISPH_REQUIRE(n == 0 || (P->x && P->type && P->vfrac && v && rho), "isph_status_dist: x, type, vfrac, v and rho are needed");
    ISPH_CHECK(stage(ctx, P->x, 3 * n, on_device, sx, &dx));
    ISPH_CHECK(stage(ctx, P->type, n, on_device, stype, &dtype));
    ISPH_CHECK(stage(ctx, P->vfrac, n, on_device, svf, &dvf));
    ISPH_CHECK(stage(ctx, v, 3 * n, on_device, sv, &dv));
    ISPH_CHECK(stage(ctx, rho, n, on_device, srho, &drho));
    return ISPH_SUCCESS;
  };
  ISPH_CHECK(step_agree(ctx, "isph_status_dist", local()));
  return status_dist_device(ctx, P->nlocal, type_mask, dx, dtype, dvf, dv, drho, centre, radius, out);
}

int isph_tgv_error_dist(isph_ctx *ctx, int nlocal, int dim, const double *x, const double *vnp1, const double *p,
                        const double *rho, const double *nu, double t, double umax, double out[4], int on_device) {
  using namespace isph;
  ISPH_REQUIRE(ctx && out, "NULL argument");
  DevTmp<double> sx, sv, sp, srho, snu;
  const double *dx = nullptr, *dv = nullptr, *dp = nullptr, *drho = nullptr, *dnu = nullptr;
  auto local = [&]() -> int {
    ISPH_REQUIRE(nlocal >= 0 && (dim == 2 || dim == 3), "isph_tgv_error_dist: need nlocal >= 0 and dim 2 or 3");
    ISPH_REQUIRE(nlocal == 0 || (x && vnp1 && p && rho && nu), "NULL argument");
    const size_t n = (size_t)nlocal;
    ISPH_CHECK(stage(ctx, x, 3 * n, on_device, sx, &dx));
    ISPH_CHECK(stage(ctx, vnp1, 3 * n, on_device, sv, &dv));
    ISPH_CHECK(stage(ctx, p, n, on_device, sp, &dp));
    ISPH_CHECK(stage(ctx, rho, n, on_device, srho, &drho));
    ISPH_CHECK(stage(ctx, nu, n, on_device, snu, &dnu));
    return ISPH_SUCCESS;
  };
  ISPH_CHECK(step_agree(ctx, "isph_tgv_error_dist", local()));
  return tgv_error_dist_device(ctx, nlocal, dx, dv, dp, drho, dnu, t, umax, out);
}

}  // extern "C"
