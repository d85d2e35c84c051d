// chebyshev.hpp -- Chebyshev polynomial in D^-1 A: the "Chebyshev" / "MLS" smoother of the SA-AMG (amg.hpp) and the
// stand-alone preconditioner isph_prec_create_chebyshev ("Precond Type" = "Chebyshev" of PrecondWrapper_Ifpack).
//
// The recurrence is Ifpack_Chebyshev::ApplyInverse / ML_Cheby restated from the packages' algorithm (Trilinos is not
// vendored: unpinned against them):
//     lambda = rho = ||D^-1 A||_inf (all-reduced maximum on several ranks; eig_type 1: min(rho, the Arnoldi estimate of
//     eig_estimate.hpp)), beta = 1.1 lambda, alpha = lambda / ratio,
//     theta = (beta + alpha) / 2, delta = (beta - alpha) / 2, sigma = theta / delta, rho_0 = 1 / sigma
//     step 1:        w = (1/theta) D^-1 (b - A y),                              y += w
//     step k = 2..d: rho_k = 1 / (2 sigma - rho_{k-1}),
//                    w = rho_k rho_{k-1} w + (2 rho_k / delta) D^-1 (b - A y),  y += w
// Every step is  w = c1 w + c2 D^-1 (b - A y),  y += w  with two scalars the host computes in double and passes as kernel
// arguments.  No dependency chain, no set-up beyond the diagonal, no dependence on the row order, the block size or
// the rank count -- and a fixed linear operator, so CG may use it.
//
// One step is ONE sweep of the matrix (k_sell_cheby_step: the slice walk of k_sell_spmv16 / k_sell_spmv with the update
// in the epilogue); the product-free first step of a zero guess (and of a residual the caller already holds) is a
// streaming kernel (k_cheby_first).  ISPH_CHEB_UNFUSED=1 (read at set-up) runs the same recurrence as
// spmv_dev(.., badd = b, alpha = -1) plus a streaming update: the cross-check and the timing baseline of the fused step.
//
// value_bits = 32: the polynomial of A~ = fl32(A).  Set-up rounds every stored value of A to the nearest float into a
// plane of its own (k_cheby_round: same element positions as S.val, 4 B per stored entry, owned by the Cheb), and D^-1,
// rho, the interval and the scalars all come from that plane; the sweeps then stream 4 B instead of 8 B of value per
// entry, convert to double and run the fma chain of the double kernel in the same order.  Vectors, accumulators and
// the update stay double: the result is the fp64 recurrence on A~, a fixed linear operator like the one on A.
// 100^3: 147.8 against 207.1 us per step for 0.62 of the bytes -- no longer HBM-bound.
//
// vec_bits = 32 (the smoother of the cycle_bits = 32 V cycle of amg.hpp; implies value_bits 32): the vectors are float too --
// y, b, w and D^-1 = fl32(1 / a~_ii).  Every kernel widens its operands, does the arithmetic of the double kernel in fp64
// (a product of two floats is exact there) and rounds once per stored element: w = fl32(wn), yout = fl32(y + wn) with the
// unrounded increment wn.  The gather of y is a 4-byte load; ghost values arrive as doubles that hold floats.
//
// K = 2..4 vectors per sweep (cheb_apply_multi; isph_prec_apply_multi, the lockstep solve, the block solve): the fused step
// and the first step restated over K double vectors -- values, columns and D^-1 loaded once, every vector its own gather,
// its own fma chains and the shared epilogue, so each vector has the bits of its own cheb_apply.  No halo form, no unfused
// form, no float-vector form: those apply one vector after the other.  100^3, K = 3: one step 416.0 us against 557.6 for
// three single steps (0.75; the algorithmic bytes say 0.64), chebyshev3 904.6 against 1239.3 us.
#pragma once
#include <cfloat>
#include <type_traits>
#include "eig_estimate.hpp"
#include "solver.hpp"

namespace isph {

constexpr int kChebMaxDegree = 16;

struct Cheb {
  int n = 0, degree = 1, unfused = 0, value_bits = 64;
  int vec_bits = 64;                                 // 32: float vectors (dinv32, w32, t32); dinv, w, t are then not kept
  double lambda = 0.0, alpha = 0.0, beta = 0.0;
  double rho = 0.0;                                  // ||D^-1 A||_inf (all-reduced), whatever lambda came from
  int eig_type = 0, eig_steps = 0;                   // eig_type 1: lambda = min(Arnoldi estimate, rho) after eig_steps steps
  // what cheb_setup was asked for (isph_prec_refactor asks for the same on the new values)
  double ratio_in = 0.0, lambda_max_in = 0.0, lambda_min_in = 0.0;
  int eig_type_in = 0, eig_iters_in = 10;
  bool held = false;   // a stand-alone preconditioner created while isph_ctx_hold_pattern was on: isph_prec_refactor takes it
  double c1[kChebMaxDegree], c2[kChebMaxDegree];   // step k (0-based): w = c1[k] w + c2[k] D^-1 (b - A y)
  DevBuf<double> dinv, w, t, r;                      // 1 / a_ii; the increment; the second y of the ping-pong; unfused: b - A y
  DevBuf<float> val32;                               // value_bits 32: fl32 of S.val, position by position (padding 0)
  DevBuf<float> dinv32, w32, t32;                    // vec_bits 32: fl32(1 / a~_ii), the increment, the second y
  // cheb_apply_multi: the increments and the second y's of K vectors, vector k at k * multi_ld().  Taken from the pool at
  // the first K-vector application, grown when a larger K comes, released with the polynomial; w and t above stay the
  // single application's own, so that one after a K-vector one finds what it always found.
  mutable DevBuf<double> wm, tm;
  size_t multi_ld() const { return ((size_t)(n > 0 ? n : 1) + 64 + 1) & ~(size_t)1; }   // even: every vector 16-byte aligned
};

// the vectors of the polynomial by their type
template <class XT> struct ChebVecs;
template <> struct ChebVecs<double> {
  static const double *dinv(const Cheb *C) { return C->dinv.p; }
  static double *w(const Cheb *C) { return C->w.p; }
  static double *t(const Cheb *C) { return C->t.p; }
};
template <> struct ChebVecs<float> {
  static const float *dinv(const Cheb *C) { return C->dinv32.p; }
  static float *w(const Cheb *C) { return C->w32.p; }
  static float *t(const Cheb *C) { return C->t32.p; }
};


inline void cheb_destroy(Cheb *C) {
  if (!C) return;
  C->dinv.release(); C->w.release(); C->t.release(); C->r.release(); C->val32.release();
  C->dinv32.release(); C->w32.release(); C->t32.release();
  C->wm.release(); C->tm.release();
  delete C;
}

// the 2d scalars of the recurrence (double, host)
inline void cheb_coefficients(Cheb *C) {
  const double theta = 0.5 * (C->beta + C->alpha), delta = 0.5 * (C->beta - C->alpha), sigma = theta / delta;
  double rho_old = 1.0 / sigma;
  C->c1[0] = 0.0;
  C->c2[0] = 1.0 / theta;
  for (int k = 1; k < C->degree; ++k) {
    const double rho_new = 1.0 / (2.0 * sigma - rho_old);
    C->c1[k] = rho_new * rho_old;
    C->c2[k] = 2.0 * rho_new / delta;
    rho_old = rho_new;
  }
}

// the one expression of the update, shared by the fused and the unfused kernels (same bits from the same operands)
__device__ __forceinline__ double cheb_increment(double c1, double c2, double w_old, double dinv, double r) {
  const double t = dinv * r;
  return fma(c1, w_old, c2 * t);
}

// ---- value_bits 32: the float plane.  v32[p] = (float)val[p] (round to nearest even, subnormals kept) for every stored
// position, padding included (0 stays 0); out[2] = 1 when a magnitude exceeds FLT_MAX.  n2 = stored / 2 (a slice holds a
// multiple of 128 entries), one double2 in and one float2 out per trip.
__global__ __launch_bounds__(kBlock) void k_cheby_round(long long n2, const double *__restrict__ val, float *__restrict__ v32,
                                                        unsigned long long *__restrict__ out) {
  const double2 *__restrict__ in = reinterpret_cast<const double2 *>(val);
  float2 *__restrict__ o = reinterpret_cast<float2 *>(v32);
  bool over = false;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (long long)gridDim.x * blockDim.x) {
    const double2 v = in[i];
    over = over || fabs(v.x) > (double)FLT_MAX || fabs(v.y) > (double)FLT_MAX;
    float2 f;
    f.x = (float)v.x;
    f.y = (float)v.y;
    o[i] = f;
  }
  if (over) atomicMax(&out[2], 1ull);
}

// ---- set-up: 1 / a_ii, rho = max_i sum_j |a_ij| / |a_ii| (ghost columns included: the row is the row of the global
// matrix, whichever rank owns its columns), a flag for a zero diagonal.  One wave per slice, lane == row.
// out[0]: bit pattern of rho (a non-negative double orders like its bits), out[1]: 1 when a diagonal entry is zero.
// empty_ok: a row without any entry (coarse operators of the AMG can have them) gets dinv = 0 and is left alone.
// VT = float: the values of the float plane, widened -- the diagonal and rho of fl32(A).
template <class VT>
__global__ __launch_bounds__(kBlock) void k_cheby_setup(int nrow, int nslices, const long long *__restrict__ slice_off,
                                                        const int *__restrict__ scol, const VT *__restrict__ sval,
                                                        int empty_ok, double *__restrict__ dinv,
                                                        unsigned long long *__restrict__ out) {
  const int slice = blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6);
  if (slice >= nslices) return;
  const int lane = threadIdx.x & 63, row = slice * kSlice + lane;
  const long long off = slice_off[slice];
  const int w = (int)((slice_off[slice + 1] - off) >> 6);
  double d = 0.0, s = 0.0;
  for (int k = 0; k < w; ++k) {   // padding: value 0
    const long long p = sell_pos(off, lane, k);
    const double v = (double)sval[p];
    if (scol[p] == row) d += v;
    s += fabs(v);
  }
  bool bad = false;
  double q = 0.0;
  if (row < nrow) {
    if (d != 0.0) {
      dinv[row] = 1.0 / d;
      q = s / fabs(d);
    } else {
      dinv[row] = 0.0;
      bad = !(empty_ok && s == 0.0);
    }
  }
  // wave maximum through the bit patterns (two 32-bit halves would not order: compare as 64-bit in a butterfly)
  unsigned long long bits = (unsigned long long)__double_as_longlong(q);
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long other = __shfl_xor(bits, o, 64);
    bits = other > bits ? other : bits;
  }
  if (lane == 0 && bits > out[0]) atomicMax(&out[0], bits);
  if (__ballot(bad) != 0ull && lane == 0) atomicMax(&out[1], 1ull);
}

// ---- one step in one sweep of the matrix ------------------------------------------------------------------------------
// (A y)_i by the slice walk of k_sell_spmv16 (C16: pair-interleaved SELL-64, lane == row, 16-bit windowed columns through
// the per-wave LDS table) or of k_sell_spmv (32-bit columns: the aux operators of the AMG), non-temporal matrix loads,
// XCD remap; then  w_i = c1 w_i + c2 dinv_i (b_i - (A y)_i),  yout_i = y_i + w_i.
// yout must NOT alias y: other waves still gather y.  c1 == 0 (first step): w is not read.
// VT = float: sval is the float plane (64 x float2 = 512 B per wave load), each value widened before its fma.
// XT = float (with VT = float): y, b, dinv, w and yout are float vectors, the ghost values yg doubles that hold floats.  The
// gather is a 4-byte load, the fma chain and the update are the fp64 ones, and w and yout are rounded once each in the
// store -- yout from y + wn with the unrounded increment.
template <bool C16, bool LIST, bool GHOST, class VT, class XT = double>
__global__ __launch_bounds__(kBlock) void k_sell_cheby_step(int nrow, int nslices, int nblocks_padded,
                                                            const long long *__restrict__ slice_off,
                                                            const void *__restrict__ cols, const int *__restrict__ wtab,
                                                            const VT *__restrict__ sval, const XT *__restrict__ y,
                                                            const double *__restrict__ yg, const XT *__restrict__ b,
                                                            const XT *__restrict__ dinv, XT *__restrict__ w,
                                                            XT *__restrict__ yout, double c1, double c2,
                                                            const int *__restrict__ slice_list) {
  constexpr int UNROLL = 8;
  typedef typename SellPair<VT>::type VT2;
  __shared__ int tab[C16 ? kBlock / kWave : 1][64];
  const int blk = xcd_remap(blockIdx.x, nblocks_padded);
  const int wave = threadIdx.x >> 6;
  int slice = blk * (kBlock / kWave) + wave;
  if (slice >= nslices) return;
  if (LIST) slice = slice_list[slice];
  const int lane = threadIdx.x & 63;
  if (C16) {
    tab[wave][lane] = wtab[(long long)slice * 64 + lane] << 10;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  const int *__restrict__ tw = tab[C16 ? wave : 0];
  const long long off = slice_off[slice];
  const int npair = (int)((slice_off[slice + 1] - off) >> 7);
  const VT2 *__restrict__ v = reinterpret_cast<const VT2 *>(sval + off) + lane;
  const unsigned *__restrict__ c16 = reinterpret_cast<const unsigned *>(static_cast<const unsigned short *>(cols) + off) + lane;
  const int2 *__restrict__ c32 = reinterpret_cast<const int2 *>(static_cast<const int *>(cols) + off) + lane;
  double acc0 = 0.0, acc1 = 0.0;
  int q = 0;
  for (; q + UNROLL <= npair; q += UNROLL) {
    VT2 vv[UNROLL];
    int ca[UNROLL], cb[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      vv[u].x = __builtin_nontemporal_load(&v[(q + u) * 64].x);
      vv[u].y = __builtin_nontemporal_load(&v[(q + u) * 64].y);
      if (C16) {
        ca[u] = (int)__builtin_nontemporal_load(&c16[(q + u) * 64]);
      } else {
        ca[u] = __builtin_nontemporal_load(&c32[(q + u) * 64].x);
        cb[u] = __builtin_nontemporal_load(&c32[(q + u) * 64].y);
      }
    }
    double xa[UNROLL], xb[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      if (C16) {
        const unsigned lo = (unsigned)ca[u] & 0xffffu, hi = (unsigned)ca[u] >> 16;
        xa[u] = x_at<GHOST>(y, yg, nrow, tw[lo >> 10] | (int)(lo & 1023u));
        xb[u] = x_at<GHOST>(y, yg, nrow, tw[hi >> 10] | (int)(hi & 1023u));
      } else {
        xa[u] = x_at<GHOST>(y, yg, nrow, ca[u]);
        xb[u] = x_at<GHOST>(y, yg, nrow, cb[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      acc0 = fma((double)vv[u].x, xa[u], acc0);
      acc1 = fma((double)vv[u].y, xb[u], acc1);
    }
  }
  for (; q < npair; ++q) {
    const VT2 vv = v[q * 64];
    int ca, cb;
    if (C16) {
      const unsigned cc = c16[q * 64];
      const unsigned lo = cc & 0xffffu, hi = cc >> 16;
      ca = tw[lo >> 10] | (int)(lo & 1023u);
      cb = tw[hi >> 10] | (int)(hi & 1023u);
    } else {
      const int2 cc = c32[q * 64];
      ca = cc.x;
      cb = cc.y;
    }
    acc0 = fma((double)vv.x, x_at<GHOST>(y, yg, nrow, ca), acc0);
    acc1 = fma((double)vv.y, x_at<GHOST>(y, yg, nrow, cb), acc1);
  }
  const int row = slice * kSlice + lane;
  if (row < nrow) {
    const double r = (double)b[row] - (acc0 + acc1);
    const double wn = cheb_increment(c1, c2, c1 != 0.0 ? (double)w[row] : 0.0, (double)dinv[row], r);
    w[row] = (XT)wn;
    yout[row] = (XT)((double)y[row] + wn);
  }
}

// ... for NV = 2..4 vectors in one sweep of the matrix (double vectors, no halo): the values (VT = double, or the float
// plane of value_bits 32), the columns and dinv are read once, every vector gathers its own y_k and runs the fma chains
// and the epilogue of k_sell_cheby_step (sell_rowsums_multi, cheb_increment) -- the bits of NV single steps.
// yout_k must not alias any y_j that is still gathered.
struct ChebMultiVecs {
  const double *y[4];
  const double *b[4];
  double *w[4];
  double *yout[4];
};
template <bool C16, class VT, int NV>
__global__ __launch_bounds__(kBlock) void k_sell_cheby_step_multi(int nrow, int nslices, int nblocks_padded,
                                                                  const long long *__restrict__ slice_off,
                                                                  const void *__restrict__ cols, const int *__restrict__ wtab,
                                                                  const VT *__restrict__ sval, const double *__restrict__ dinv,
                                                                  ChebMultiVecs V, double c1, double c2) {
  __shared__ int tab[C16 ? kBlock / kWave : 1][64];
  const int blk = xcd_remap(blockIdx.x, nblocks_padded);
  const int wave = threadIdx.x >> 6;
  const int slice = blk * (kBlock / kWave) + wave;
  if (slice >= nslices) return;
  const int lane = threadIdx.x & 63;
  if (C16) {
    tab[wave][lane] = wtab[(long long)slice * 64 + lane] << 10;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  const long long off = slice_off[slice];
  const int npair = (int)((slice_off[slice + 1] - off) >> 7);
  double sum[NV];
  sell_rowsums_multi<C16, VT, NV>(tab[C16 ? wave : 0], off, npair, lane, cols, sval, V.y, sum);
  const int row = slice * kSlice + lane;
  if (row < nrow) {
    const double d = dinv[row];
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const double r = V.b[k][row] - sum[k];
      const double wn = cheb_increment(c1, c2, c1 != 0.0 ? V.w[k][row] : 0.0, d, r);
      V.w[k][row] = wn;
      V.yout[k][row] = V.y[k][row] + wn;
    }
  }
}

// ---- streaming kernels ------------------------------------------------------------------------------------------------
// The product-free first step:  w = c2 D^-1 r,  yout = yin + w  (yin == NULL: the zero guess, yout = w).  r is b for a
// zero guess, or a residual b - A yin the caller already holds.  VEC: 16-byte loads and stores (all pointers aligned).
template <bool VEC>
__global__ __launch_bounds__(kBlock) void k_cheby_first(int n, double c2, const double *__restrict__ dinv,
                                                        const double *__restrict__ r, const double *yin,
                                                        double *__restrict__ w, double *yout) {
  const long long stride = (long long)gridDim.x * blockDim.x, t0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (VEC) {
    const long long n2 = n >> 1;
    const double2 *d2 = reinterpret_cast<const double2 *>(dinv), *r2 = reinterpret_cast<const double2 *>(r);
    const double2 *y2 = reinterpret_cast<const double2 *>(yin);
    double2 *w2 = reinterpret_cast<double2 *>(w), *o2 = reinterpret_cast<double2 *>(yout);
    for (long long i = t0; i < n2; i += stride) {
      const double2 d = d2[i], rr = r2[i];
      double2 wn, yo;
      wn.x = cheb_increment(0.0, c2, 0.0, d.x, rr.x);
      wn.y = cheb_increment(0.0, c2, 0.0, d.y, rr.y);
      yo = wn;
      if (yin) { const double2 yy = y2[i]; yo.x = yy.x + wn.x; yo.y = yy.y + wn.y; }
      w2[i] = wn;
      o2[i] = yo;
    }
    if ((n & 1) && t0 == 0) {
      const int i = n - 1;
      const double wn = cheb_increment(0.0, c2, 0.0, dinv[i], r[i]);
      w[i] = wn;
      yout[i] = yin ? yin[i] + wn : wn;
    }
  } else {
    for (long long i = t0; i < n; i += stride) {
      const double wn = cheb_increment(0.0, c2, 0.0, dinv[i], r[i]);
      w[i] = wn;
      yout[i] = yin ? yin[i] + wn : wn;
    }
  }
}

// ... for NV = 2..4 vectors: dinv is read once per element.  VEC only when every one of the NV pointers of every kind is
// 16-byte aligned (the components of a block system with an odd leading dimension are not): the host decides.
struct ChebFirstVecs {
  const double *r[4];
  const double *yin[4];   // all NULL (the zero guess) or none
  double *w[4];
  double *yout[4];
};
template <bool VEC, int NV>
__global__ __launch_bounds__(kBlock) void k_cheby_first_multi(int n, double c2, const double *__restrict__ dinv, ChebFirstVecs V) {
  const long long stride = (long long)gridDim.x * blockDim.x, t0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const bool guess = V.yin[0] != nullptr;
  if (VEC) {
    const long long n2 = n >> 1;
    const double2 *d2 = reinterpret_cast<const double2 *>(dinv);
    for (long long i = t0; i < n2; i += stride) {
      const double2 d = d2[i];
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        const double2 rr = reinterpret_cast<const double2 *>(V.r[k])[i];
        double2 wn, yo;
        wn.x = cheb_increment(0.0, c2, 0.0, d.x, rr.x);
        wn.y = cheb_increment(0.0, c2, 0.0, d.y, rr.y);
        yo = wn;
        if (guess) { const double2 yy = reinterpret_cast<const double2 *>(V.yin[k])[i]; yo.x = yy.x + wn.x; yo.y = yy.y + wn.y; }
        reinterpret_cast<double2 *>(V.w[k])[i] = wn;
        reinterpret_cast<double2 *>(V.yout[k])[i] = yo;
      }
    }
    if ((n & 1) && t0 == 0) {
      const int i = n - 1;
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        const double wn = cheb_increment(0.0, c2, 0.0, dinv[i], V.r[k][i]);
        V.w[k][i] = wn;
        V.yout[k][i] = guess ? V.yin[k][i] + wn : wn;
      }
    }
  } else {
    for (long long i = t0; i < n; i += stride) {
      const double d = dinv[i];
#pragma unroll
      for (int k = 0; k < NV; ++k) {
        const double wn = cheb_increment(0.0, c2, 0.0, d, V.r[k][i]);
        V.w[k][i] = wn;
        V.yout[k][i] = guess ? V.yin[k][i] + wn : wn;
      }
    }
  }
}

// ... of float vectors (vec_bits 32): the same step with every operand widened, fp64 arithmetic, w and yout rounded once.
// VEC: 16-byte loads and stores carry 4 floats per lane; the up to 3 elements behind the last quad go one by one.
template <bool VEC>
__global__ __launch_bounds__(kBlock) void k_cheby_first_f32(int n, double c2, const float *__restrict__ dinv,
                                                            const float *__restrict__ r, const float *yin,
                                                            float *__restrict__ w, float *yout) {
  const long long stride = (long long)gridDim.x * blockDim.x, t0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (VEC) {
    const long long n4 = n >> 2;
    const float4 *d4 = reinterpret_cast<const float4 *>(dinv), *r4 = reinterpret_cast<const float4 *>(r);
    const float4 *y4 = reinterpret_cast<const float4 *>(yin);
    float4 *w4 = reinterpret_cast<float4 *>(w), *o4 = reinterpret_cast<float4 *>(yout);
    for (long long i = t0; i < n4; i += stride) {
      const float4 d = d4[i], rr = r4[i];
      const double wx = cheb_increment(0.0, c2, 0.0, (double)d.x, (double)rr.x);
      const double wy = cheb_increment(0.0, c2, 0.0, (double)d.y, (double)rr.y);
      const double wz = cheb_increment(0.0, c2, 0.0, (double)d.z, (double)rr.z);
      const double ww = cheb_increment(0.0, c2, 0.0, (double)d.w, (double)rr.w);
      float4 wn, yo;
      wn.x = (float)wx; wn.y = (float)wy; wn.z = (float)wz; wn.w = (float)ww;
      yo = wn;
      if (yin) {
        const float4 yy = y4[i];
        yo.x = (float)((double)yy.x + wx); yo.y = (float)((double)yy.y + wy);
        yo.z = (float)((double)yy.z + wz); yo.w = (float)((double)yy.w + ww);
      }
      w4[i] = wn;
      o4[i] = yo;
    }
    const int i = (n & ~3) + (int)t0;
    if (t0 < 3 && i < n) {
      const double wn = cheb_increment(0.0, c2, 0.0, (double)dinv[i], (double)r[i]);
      w[i] = (float)wn;
      yout[i] = yin ? (float)((double)yin[i] + wn) : (float)wn;
    }
  } else {
    for (long long i = t0; i < n; i += stride) {
      const double wn = cheb_increment(0.0, c2, 0.0, (double)dinv[i], (double)r[i]);
      w[i] = (float)wn;
      yout[i] = yin ? (float)((double)yin[i] + wn) : (float)wn;
    }
  }
}

// ISPH_CHEB_UNFUSED=1: the update behind a separate r = b - A y (r is a double vector for either XT: the product's
// residual is not rounded on its way here, as it is not inside the fused step)
template <class XT = double>
__global__ __launch_bounds__(kBlock) void k_cheby_update(int n, double c1, double c2, const XT *__restrict__ dinv,
                                                         const double *__restrict__ r, XT *__restrict__ w,
                                                         const XT *yin, XT *yout) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const double wn = cheb_increment(c1, c2, c1 != 0.0 ? (double)w[i] : 0.0, (double)dinv[i], r[i]);
    w[i] = (XT)wn;
    yout[i] = (XT)((double)yin[i] + wn);
  }
}

// float vectors in and out of the fp64 world: out = fl32(in) (round to nearest even; the residual that enters the
// cycle_bits = 32 V cycle, the float D^-1; flag != NULL: flag[2] = 1 when a magnitude exceeds FLT_MAX) and out = in widened
// (the cycle's result, the coarsest right-hand side of several ranks)
__global__ __launch_bounds__(kBlock) void k_cheby_narrow(long long n, const double *__restrict__ in, float *__restrict__ out,
                                                         unsigned long long *__restrict__ flag) {
  bool over = false;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const double v = in[i];
    over = over || fabs(v) > (double)FLT_MAX;
    out[i] = (float)v;
  }
  if (flag != nullptr && over) atomicMax(&flag[2], 1ull);
}
__global__ __launch_bounds__(kBlock) void k_cheby_widen(long long n, const float *__restrict__ in, double *__restrict__ out) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    out[i] = (double)in[i];
}

// the float plane of `count` doubles (count even: k_cheby_round, a pair per trip; an odd last element: k_cheby_narrow)
inline void cheb_round_plane(isph_ctx *ctx, long long count, const double *val, float *v32, unsigned long long *flag) {
  if (count >= 2)
    hipLaunchKernelGGL(k_cheby_round, dim3(stream_grid(count / 2)), dim3(kBlock), 0, ctx->stream, count / 2, val, v32, flag);
  if (count & 1)
    hipLaunchKernelGGL(k_cheby_narrow, dim3(1), dim3(kBlock), 0, ctx->stream, 1LL, val + (count - 1), v32 + (count - 1), flag);
}

// ---- host side --------------------------------------------------------------------------------------------------------
// 1 / a_ii of every row into dinv and the rank's own rho = max_i sum_j |a_ij| / |a_ii| (k_cheby_setup on the double values,
// rows without a diagonal: dinv = 0): what the eigenvalue estimate of an AMG level needs before any polynomial exists.
inline int cheb_diag_rho(isph_ctx *ctx, const isph_mat *A, DevBuf<double> &dinv, double *rho) {
  const Sell &S = A->S;
  DevTmp<unsigned long long> flag;
  ISPH_CHECK(flag.reserve(3));
  ISPH_CHECK(dinv.reserve((size_t)(S.nrow > 0 ? S.nrow : 1) + 64));
  ISPH_CHECK_HIP(hipMemsetAsync(flag.p, 0, 3 * sizeof(unsigned long long), ctx->stream));
  if (S.nslices > 0)
    hipLaunchKernelGGL((k_cheby_setup<double>), dim3((S.nslices + 3) / 4), dim3(kBlock), 0, ctx->stream, S.nrow, S.nslices,
                       (const long long *)S.slice_off.p, (const int *)S.col.p, (const double *)S.val.p, 1, dinv.p, flag.p);
  unsigned long long hb = 0ull;
  ISPH_CHECK_HIP(hipMemcpyAsync(&hb, flag.p, sizeof(hb), hipMemcpyDeviceToHost, ctx->stream));
  ISPH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  ISPH_CHECK_HIP(hipGetLastError());
  memcpy(rho, &hb, sizeof(double));
  return ISPH_SUCCESS;
}

// collective: every rank of the context calls this together (stand-alone: a context with a communicator; AMG: a
// hierarchy across ranks) -- rho is the all-reduced maximum and a failure on one rank is a failure on all.
// prior_failure: this rank has already failed and only takes part in the collective step.
// value_bits: 64, or 32 = the polynomial of fl32(A) (the caller has checked the value).
// eig_type 1 (with lambda_max <= 0): lambda is the clipped Arnoldi estimate of eig_estimate.hpp after eig_iters steps on
// the operator the sweeps apply (the float plane with value_bits 32), start vector of `eig_level`; collective like rho.
// vec_bits 32 (takes value_bits 32 with it): float vectors.  The plane, rho, the estimate and the scalars are those of
// value_bits 32; then D^-1 is rounded into dinv32 (a quotient beyond FLT_MAX fails like a value beyond it) and the double
// one goes back to the pool.  w, t of the double polynomial are never reserved.
inline int cheb_setup(isph_ctx *ctx, const isph_mat *A, int degree, double ratio, double lambda_max, double lambda_min,
                      bool empty_ok, bool collective, bool prior_failure, Cheb **out, int value_bits = 64, int eig_type = 0,
                      int eig_iters = 10, int eig_level = 0, int vec_bits = 64) {
  const Sell &S = A->S;
  int rc = ISPH_SUCCESS;
  Cheb *C = new Cheb();
  C->n = S.nrow;
  C->degree = degree;
  C->ratio_in = ratio; C->lambda_max_in = lambda_max; C->lambda_min_in = lambda_min;
  C->eig_type_in = eig_type; C->eig_iters_in = eig_iters;
  C->vec_bits = vec_bits == 32 ? 32 : 64;
  C->value_bits = (value_bits == 32 || C->vec_bits == 32) ? 32 : 64;
  const bool f32 = C->value_bits == 32, v32 = C->vec_bits == 32;
  const char *env = getenv("ISPH_CHEB_UNFUSED");
  C->unfused = env && env[0] == '1';
  DevTmp<unsigned long long> flag;
  double rho = 0.0;
  if (!prior_failure) {
    const size_t m = (size_t)(S.nrow > 0 ? S.nrow : 1) + 64;
    rc = flag.reserve(3);
    if (rc == ISPH_SUCCESS) rc = C->dinv.reserve(m);
    if (rc == ISPH_SUCCESS && f32) rc = C->val32.reserve((size_t)(S.stored > 0 ? S.stored : 1));
    if (rc == ISPH_SUCCESS && !v32) rc = C->w.reserve(m);
    if (rc == ISPH_SUCCESS && !v32) rc = C->t.reserve(m);
    if (rc == ISPH_SUCCESS && v32) rc = C->dinv32.reserve(m);
    if (rc == ISPH_SUCCESS && v32) rc = C->w32.reserve(m);
    if (rc == ISPH_SUCCESS && v32) rc = C->t32.reserve(m);
    if (rc == ISPH_SUCCESS && C->unfused) rc = C->r.reserve(m);
    if (rc == ISPH_SUCCESS && hipMemsetAsync(flag.p, 0, 3 * sizeof(unsigned long long), ctx->stream) != hipSuccess)
      rc = fail("memset failed", __FILE__, __LINE__);
    unsigned long long hb[3] = {0ull, 0ull, 0ull};
    if (rc == ISPH_SUCCESS) {
      if (f32 && S.stored > 0)   // one streaming pass over S.val; the set-up kernel below then reads the plane
        hipLaunchKernelGGL(k_cheby_round, dim3(stream_grid(S.stored / 2)), dim3(kBlock), 0, ctx->stream, S.stored / 2, (const double *)S.val.p, C->val32.p, flag.p);
      if (S.nslices > 0 && f32)
        hipLaunchKernelGGL((k_cheby_setup<float>), dim3((S.nslices + 3) / 4), dim3(kBlock), 0, ctx->stream, S.nrow, S.nslices,
                           (const long long *)S.slice_off.p, (const int *)S.col.p, (const float *)C->val32.p, empty_ok ? 1 : 0,
                           C->dinv.p, flag.p);
      else if (S.nslices > 0)
        hipLaunchKernelGGL((k_cheby_setup<double>), dim3((S.nslices + 3) / 4), dim3(kBlock), 0, ctx->stream, S.nrow, S.nslices,
                           (const long long *)S.slice_off.p, (const int *)S.col.p, (const double *)S.val.p, empty_ok ? 1 : 0,
                           C->dinv.p, flag.p);
      if (hipMemcpyAsync(hb, flag.p, sizeof(hb), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
          hipStreamSynchronize(ctx->stream) != hipSuccess || hipGetLastError() != hipSuccess)
        rc = fail("Chebyshev set-up failed", __FILE__, __LINE__);
    }
    if (rc == ISPH_SUCCESS && hb[2] != 0ull)
      rc = fail("Chebyshev: a matrix value exceeds the range of single precision (value_bits = 32 rounds the values to float)", __FILE__, __LINE__);
    if (rc == ISPH_SUCCESS && hb[1] != 0ull)
      rc = fail("Chebyshev: the matrix has a zero diagonal entry (the polynomial acts on D^-1 A)", __FILE__, __LINE__);
    memcpy(&rho, &hb[0], sizeof(double));
  }
  if (prior_failure) rc = ISPH_FAILURE;   // what this rank brings to the vote
  // (a rank that has failed keeps its message whatever becomes of the all-reduce)
  comm_consensus(ctx, collective, "Chebyshev", rc == ISPH_SUCCESS ? "Chebyshev: the all-reduce of rho failed" : nullptr, &rho, 1, rc);
  if (rc != ISPH_SUCCESS) { cheb_destroy(C); return rc; }
  C->rho = rho;
  C->lambda = lambda_max > 0.0 ? lambda_max : rho;
  if (eig_type == 1 && !(lambda_max > 0.0)) {
    // (every rank is here or none: a failure above has been all-reduced)
    EigResult e;
    rc = eig_estimate(ctx, A, f32 ? (const float *)C->val32.p : nullptr, C->dinv.p, C->rho, eig_iters, eig_level, eig_unfused_env(),
                      collective, &e);
    if (rc != ISPH_SUCCESS) { cheb_destroy(C); return rc; }
    C->eig_type = 1;
    C->eig_steps = e.steps;
    C->lambda = e.lambda_used;
  }
  if (!(C->lambda > 0.0)) C->lambda = 1.0;   // a level without entries: D^-1 A is empty, any interval does
  C->beta = 1.1 * C->lambda;
  C->alpha = lambda_min > 0.0 ? lambda_min : C->lambda / ratio;
  if (!(C->alpha < C->beta)) { cheb_destroy(C); return fail("Chebyshev: lambda_min must be below 1.1 lambda_max", __FILE__, __LINE__); }
  cheb_coefficients(C);
  if (v32) {   // (rank-local and after the last collective step: a failure here is agreed on by the caller's own consensus)
    unsigned long long hb[3] = {0ull, 0ull, 0ull};
    if (hipMemsetAsync(flag.p, 0, 3 * sizeof(unsigned long long), ctx->stream) != hipSuccess) rc = fail("memset failed", __FILE__, __LINE__);
    if (rc == ISPH_SUCCESS && S.nrow > 0)
      hipLaunchKernelGGL(k_cheby_narrow, dim3(stream_grid(S.nrow)), dim3(kBlock), 0, ctx->stream, (long long)S.nrow,
                         (const double *)C->dinv.p, C->dinv32.p, flag.p);
    if (rc == ISPH_SUCCESS && (hipMemcpyAsync(hb, flag.p, sizeof(hb), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
                               hipStreamSynchronize(ctx->stream) != hipSuccess || hipGetLastError() != hipSuccess))
      rc = fail("Chebyshev set-up failed", __FILE__, __LINE__);
    if (rc == ISPH_SUCCESS && hb[2] != 0ull)
      rc = fail("Chebyshev: the inverse of a diagonal entry exceeds the range of single precision (cycle_bits = 32 stores D^-1 as float)", __FILE__, __LINE__);
    if (rc != ISPH_SUCCESS) { cheb_destroy(C); return rc; }
    C->dinv.release();
  }
  *out = C;
  return ISPH_SUCCESS;
}

template <bool LIST, bool GHOST, class VT, class XT>
inline void cheb_step_launch(isph_ctx *ctx, const Sell &S, bool c16, int nsl, const int *list, const Cheb *C, const VT *val,
                             const XT *b, const XT *y, const double *yg, XT *yout, double c1, double c2) {
  if (nsl <= 0) return;
  int nbp = 0;
  const int grid = spmv_grid(nsl, &nbp);
  if (c16)
    hipLaunchKernelGGL((k_sell_cheby_step<true, LIST, GHOST, VT, XT>), dim3(grid), dim3(kBlock), 0, ctx->stream, S.nrow, nsl, nbp,
                       (const long long *)S.slice_off.p, (const void *)S.col16.p, (const int *)S.wtab.p, val, y, yg,
                       b, ChebVecs<XT>::dinv(C), ChebVecs<XT>::w(C), yout, c1, c2, list);
  else
    hipLaunchKernelGGL((k_sell_cheby_step<false, LIST, GHOST, VT, XT>), dim3(grid), dim3(kBlock), 0, ctx->stream, S.nrow, nsl, nbp,
                       (const long long *)S.slice_off.p, (const void *)S.col.p, (const int *)nullptr, val, y, yg,
                       b, ChebVecs<XT>::dinv(C), ChebVecs<XT>::w(C), yout, c1, c2, list);
}

// the fused sweep over the double values of the matrix or over the float plane of the preconditioner
template <class VT, class XT>
inline int cheb_step_fused(isph_ctx *ctx, const isph_mat *A, const Cheb *C, const VT *val, bool halo, bool c16, const XT *b,
                           const XT *y, XT *yout, double c1, double c2) {
  const Sell &S = A->S;
  if (!halo) {
    cheb_step_launch<false, false, VT, XT>(ctx, S, c16, S.nslices, nullptr, C, val, b, y, nullptr, yout, c1, c2);
  } else {
    const isph_halo &H = A->halo;
    ISPH_CHECK(halo_begin(ctx, A, y));
    cheb_step_launch<true, false, VT, XT>(ctx, S, c16, H.n_int, H.list_int.p, C, val, b, y, nullptr, yout, c1, c2);
    ISPH_CHECK_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_halo, 0));
    cheb_step_launch<true, true, VT, XT>(ctx, S, c16, H.n_bnd, H.list_bnd.p, C, val, b, y, ctx->xghost.p, yout, c1, c2);
  }
  return ISPH_SUCCESS;
}

// r = b - A y of the unfused step, a double vector whatever the vectors are (float vectors: the product of the float plane
// with the float y, the fp64 row sum subtracted from the widened b and stored unrounded)
inline int cheb_unfused_residual(isph_ctx *ctx, const isph_mat *A, const Cheb *C, const double *b, const double *y) {
  return spmv_dev(ctx, A, y, C->r.p, nullptr, b, -1.0, C->value_bits == 32 ? (const float *)C->val32.p : nullptr);
}
inline int cheb_unfused_residual(isph_ctx *ctx, const isph_mat *A, const Cheb *C, const float *b, const float *y) {
  return spmv_dev_f32<double>(ctx, A, (const float *)C->val32.p, y, C->r.p, b, -1.0);
}

// one step with a matrix product: yout = y + w, w = c1 w + c2 D^-1 (b - A y); yout != y.  With a halo plan the exchange
// of y overlaps the interior slices exactly as in spmv_dev.  XT = float: the polynomial of float vectors (vec_bits 32).
template <class XT>
inline int cheb_step(isph_ctx *ctx, const isph_mat *A, const Cheb *C, const XT *b, const XT *y, XT *yout, double c1,
                     double c2) {
  const Sell &S = A->S;
  constexpr bool v32 = std::is_same<XT, float>::value;
  if (C->unfused) {
    // r = b - A y (value_bits 32: the product reads the float plane)
    ISPH_CHECK(cheb_unfused_residual(ctx, A, C, b, y));
    hipLaunchKernelGGL((k_cheby_update<XT>), dim3(stream_grid(S.nrow)), dim3(kBlock), 0, ctx->stream, S.nrow, c1, c2,
                       ChebVecs<XT>::dinv(C), (const double *)C->r.p, ChebVecs<XT>::w(C), y, yout);
    ISPH_CHECK_HIP(hipGetLastError());
    return ISPH_SUCCESS;
  }
  ProfScope prof((A->local || A->aux) ? nullptr : ctx, PROF_SPMV);   // a sweep of the caller's operator, like spmv_dev's
  const bool halo = !A->local && (S.ncol != S.nrow || A->halo.nsend > 0);
  const bool c16 = !A->local && !A->aux && sell_cols16(ctx, S);
  if constexpr (v32) {   // (float vectors only ever meet the float plane)
    ISPH_CHECK((cheb_step_fused<float, XT>(ctx, A, C, (const float *)C->val32.p, halo, c16, b, y, yout, c1, c2)));
  } else {
    if (C->value_bits == 32) ISPH_CHECK((cheb_step_fused<float, XT>(ctx, A, C, (const float *)C->val32.p, halo, c16, b, y, yout, c1, c2)));
    else ISPH_CHECK((cheb_step_fused<double, XT>(ctx, A, C, (const double *)S.val.p, halo, c16, b, y, yout, c1, c2)));
  }
  ISPH_CHECK_HIP(hipGetLastError());
  return ISPH_SUCCESS;
}

inline void cheb_first_launch(isph_ctx *ctx, const Cheb *C, const double *r, const double *yin, double *yout) {
  const int n = C->n;
  if (n <= 0) return;
  const uintptr_t bits = reinterpret_cast<uintptr_t>(r) | reinterpret_cast<uintptr_t>(yin) | reinterpret_cast<uintptr_t>(yout);
  if ((bits & 15) == 0)   // (dinv and w are buffers of the pool)
    hipLaunchKernelGGL((k_cheby_first<true>), dim3(stream_grid((n + 1) / 2)), dim3(kBlock), 0, ctx->stream, n, C->c2[0],
                       (const double *)C->dinv.p, r, yin, C->w.p, yout);
  else
    hipLaunchKernelGGL((k_cheby_first<false>), dim3(stream_grid(n)), dim3(kBlock), 0, ctx->stream, n, C->c2[0],
                       (const double *)C->dinv.p, r, yin, C->w.p, yout);
}
inline void cheb_first_launch(isph_ctx *ctx, const Cheb *C, const float *r, const float *yin, float *yout) {
  const int n = C->n;
  if (n <= 0) return;
  const uintptr_t bits = reinterpret_cast<uintptr_t>(r) | reinterpret_cast<uintptr_t>(yin) | reinterpret_cast<uintptr_t>(yout);
  if ((bits & 15) == 0)   // (dinv32 and w32 are buffers of the pool)
    hipLaunchKernelGGL((k_cheby_first_f32<true>), dim3(stream_grid((n + 3) / 4)), dim3(kBlock), 0, ctx->stream, n, C->c2[0],
                       (const float *)C->dinv32.p, r, yin, C->w32.p, yout);
  else
    hipLaunchKernelGGL((k_cheby_first_f32<false>), dim3(stream_grid(n)), dim3(kBlock), 0, ctx->stream, n, C->c2[0],
                       (const float *)C->dinv32.p, r, yin, C->w32.p, yout);
}

// y <- y + p(D^-1 A) D^-1 (b - A y), p of degree C->degree.
//   zero_guess: y is not read (y = p(D^-1 A) D^-1 b); the first step makes no matrix product.
//   r0 != NULL (with a guess): b - A y is already there (the AMG cycle's A P shortcut); again no product in step 1.
// The steps ping-pong between y and C->t; the result is in y for every degree.
// XT = float: a polynomial set up with vec_bits 32, on float vectors (t32 is the second y).
template <class XT>
inline int cheb_apply(isph_ctx *ctx, const isph_mat *A, const Cheb *C, const XT *b, XT *y, bool zero_guess,
                      const XT *r0 = nullptr) {
  ISPH_REQUIRE(C != nullptr && C->n == A->S.nrow, "Chebyshev: not set up for this matrix");
  ISPH_REQUIRE(C->vec_bits == (int)(8 * sizeof(XT)), "Chebyshev: set up for vectors of the other precision");
  const int d = C->degree;
  const size_t nbytes = sizeof(XT) * (size_t)(C->n > 0 ? C->n : 0);
  XT *T = ChebVecs<XT>::t(C);
  const XT *cur;
  int k0;   // first step that needs a product
  if (zero_guess || r0) {
    // d - 1 products follow: an even number ends where it starts
    XT *first = ((d - 1) % 2 == 0) ? y : T;
    cheb_first_launch(ctx, C, zero_guess ? b : r0, zero_guess ? (const XT *)nullptr : (const XT *)y, first);
    cur = first;
    k0 = 1;
  } else {
    cur = y;
    k0 = 0;
  }
  for (int k = k0; k < d; ++k) {
    XT *nxt = cur == y ? T : y;
    ISPH_CHECK(cheb_step(ctx, A, C, b, cur, nxt, C->c1[k], C->c2[k]));
    cur = nxt;
  }
  if (cur != y && nbytes > 0)   // (a guess and an odd number of products)
    ISPH_CHECK_HIP(hipMemcpyAsync(y, T, nbytes, hipMemcpyDeviceToDevice, ctx->stream));
  ISPH_CHECK_HIP(hipGetLastError());
  return ISPH_SUCCESS;
}

// ---- K vectors per sweep ----------------------------------------------------------------------------------------------
// whether cheb_apply_multi can serve this polynomial: fused steps of double vectors on a matrix without a halo
inline bool cheb_multi_ok(const isph_mat *A, const Cheb *C) {
  return C != nullptr && A != nullptr && !C->unfused && C->vec_bits == 64 && !mat_has_halo(A);
}

template <class VT>
inline void cheb_step_multi_launch(isph_ctx *ctx, const Sell &S, bool c16, int K, const VT *val, const double *dinv,
                                   const ChebMultiVecs &V, double c1, double c2) {
  if (S.nslices <= 0) return;
  int nbp = 0;
  const int grid = spmv_grid(S.nslices, &nbp);
#define ISPH_CHEB_STEP_MULTI(C16, NV, COLS, WTAB)                                                                             \
  hipLaunchKernelGGL((k_sell_cheby_step_multi<C16, VT, NV>), dim3(grid), dim3(kBlock), 0, ctx->stream, S.nrow, S.nslices, nbp, \
                     (const long long *)S.slice_off.p, (const void *)(COLS), (const int *)(WTAB), val, dinv, V, c1, c2)
  if (c16) {
    if (K == 2) ISPH_CHEB_STEP_MULTI(true, 2, S.col16.p, S.wtab.p);
    else if (K == 3) ISPH_CHEB_STEP_MULTI(true, 3, S.col16.p, S.wtab.p);
    else ISPH_CHEB_STEP_MULTI(true, 4, S.col16.p, S.wtab.p);
  } else {
    if (K == 2) ISPH_CHEB_STEP_MULTI(false, 2, S.col.p, nullptr);
    else if (K == 3) ISPH_CHEB_STEP_MULTI(false, 3, S.col.p, nullptr);
    else ISPH_CHEB_STEP_MULTI(false, 4, S.col.p, nullptr);
  }
#undef ISPH_CHEB_STEP_MULTI
}

template <bool VEC>
inline void cheb_first_multi_launch(isph_ctx *ctx, const Cheb *C, int K, int grid, const ChebFirstVecs &V) {
  const double *dinv = C->dinv.p;
  if (K == 2) hipLaunchKernelGGL((k_cheby_first_multi<VEC, 2>), dim3(grid), dim3(kBlock), 0, ctx->stream, C->n, C->c2[0], dinv, V);
  else if (K == 3) hipLaunchKernelGGL((k_cheby_first_multi<VEC, 3>), dim3(grid), dim3(kBlock), 0, ctx->stream, C->n, C->c2[0], dinv, V);
  else hipLaunchKernelGGL((k_cheby_first_multi<VEC, 4>), dim3(grid), dim3(kBlock), 0, ctx->stream, C->n, C->c2[0], dinv, V);
}

// cheb_apply for K = 2..4 double vectors, one sweep of the matrix per step for all of them: y_k <- y_k + p(D^-1 A) D^-1
// (b_k - A y_k).  The same first step, the same ping-pong parity between y_k and the second buffer (tm, vector k) and the
// same closing copy as cheb_apply, so y_k has the bits of cheb_apply(.., b_k, y_k, zero_guess, r0_k).
// r0s: NULL, or the K residuals b_k - A y_k the caller already holds (with a guess).
inline int cheb_apply_multi(isph_ctx *ctx, const isph_mat *A, const Cheb *C, int K, const double *const *bs, double *const *ys,
                            bool zero_guess, const double *const *r0s = nullptr) {
  ISPH_REQUIRE(C != nullptr && C->n == A->S.nrow, "Chebyshev: not set up for this matrix");
  ISPH_REQUIRE(K >= 2 && K <= 4 && cheb_multi_ok(A, C), "Chebyshev: no K-vector form for this polynomial, matrix or K");
  const Sell &S = A->S;
  const int d = C->degree, n = C->n;
  const size_t ld = C->multi_ld(), nbytes = sizeof(double) * (size_t)(n > 0 ? n : 0);
  ISPH_CHECK(C->wm.reserve(ld * (size_t)K));
  ISPH_CHECK(C->tm.reserve(ld * (size_t)K));
  double *W[4], *T[4];
  for (int k = 0; k < 4; ++k) { W[k] = C->wm.p + ld * (size_t)(k < K ? k : 0); T[k] = C->tm.p + ld * (size_t)(k < K ? k : 0); }
  auto at = [K](const double *const *v, int k) { return v[k < K ? k : 0]; };
  bool in_y;   // where the current iterates are: the callers' y_k, or T
  int k0;      // first step that needs a product
  if (zero_guess || r0s) {
    in_y = (d - 1) % 2 == 0;   // d - 1 products follow: an even number ends where it starts
    if (n > 0) {
      ChebFirstVecs V;
      uintptr_t bits = 0;
      for (int k = 0; k < 4; ++k) {
        V.r[k] = at(zero_guess ? bs : r0s, k);
        V.yin[k] = zero_guess ? nullptr : ys[k < K ? k : 0];
        V.w[k] = W[k];
        V.yout[k] = in_y ? ys[k < K ? k : 0] : T[k];
        bits |= reinterpret_cast<uintptr_t>(V.r[k]) | reinterpret_cast<uintptr_t>(V.yin[k]) | reinterpret_cast<uintptr_t>(V.yout[k]);
      }
      if ((bits & 15) == 0) cheb_first_multi_launch<true>(ctx, C, K, stream_grid((n + 1) / 2), V);   // (dinv, wm, tm: the pool's)
      else cheb_first_multi_launch<false>(ctx, C, K, stream_grid(n), V);
    }
    k0 = 1;
  } else {
    in_y = true;
    k0 = 0;
  }
  const bool c16 = !A->local && !A->aux && sell_cols16(ctx, S);
  for (int k = k0; k < d; ++k) {
    ProfScope prof((A->local || A->aux) ? nullptr : ctx, PROF_SPMV);   // a sweep of the caller's operator, like cheb_step's
    ChebMultiVecs V;
    for (int j = 0; j < 4; ++j) {
      double *yj = ys[j < K ? j : 0];
      V.y[j] = in_y ? yj : T[j];
      V.yout[j] = in_y ? T[j] : yj;
      V.b[j] = at(bs, j);
      V.w[j] = W[j];
    }
    if (C->value_bits == 32) cheb_step_multi_launch<float>(ctx, S, c16, K, (const float *)C->val32.p, (const double *)C->dinv.p, V, C->c1[k], C->c2[k]);
    else cheb_step_multi_launch<double>(ctx, S, c16, K, (const double *)S.val.p, (const double *)C->dinv.p, V, C->c1[k], C->c2[k]);
    in_y = !in_y;
  }
  if (!in_y && nbytes > 0)   // (a guess and an odd number of products)
    for (int k = 0; k < K; ++k) ISPH_CHECK_HIP(hipMemcpyAsync(ys[k], T[k], nbytes, hipMemcpyDeviceToDevice, ctx->stream));
  ISPH_CHECK_HIP(hipGetLastError());
  return ISPH_SUCCESS;
}

}  // namespace isph
