// svgd_interact.h -- the per-iteration particle interaction of SVGD with NO n x n matrix in LDS: ONE definition for
// svgd_big_kernel (bore_svgd.hip: the network in LDS) and stream_svgd_kernel (bore_stream.hip: the network streamed
// from global memory); svgd_kernel, whose drive reads a stored matrix, keeps its own text.  Particles x, their input gradients fg, the update grad and the Adagrad history hist are
// fp64 [n][D] in LDS, f and zeta fp64 [n]; entries of the kernel matrix are formed where they are used.  Every
// routine is called by the whole workgroup (BORE_THREADS work-items) with the same arguments, behind a barrier after
// the last write of what it reads, and ends with a barrier.  Sums run in plain index order; the only atomics are the
// integer LDS ones of the radix select.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "mlp_layout.h"

namespace bore {

#define BORE_SVGD_MAX_PARTICLES 4096

constexpr int SVGD_SELECT_WORDS = 256 + 8;  // the radix select's scratch: [256] bins + [8]

// |x_i - x_j|^2, the terms added in ascending d.  Four coordinates' loads at a time ahead of the sum: with one wave
// per SIMD nothing else hides an LDS round trip per term.
__device__ __forceinline__ double svgd_sqdist(const double *x, const int D, const int i, const int j) {
  const double *xi = x + i * D, *xj = x + j * D;
  double s = 0.0;
  int d = 0;
  for (; d + 4 <= D; d += 4) {
    const double t0 = xi[d] - xj[d], t1 = xi[d + 1] - xj[d + 1], t2 = xi[d + 2] - xj[d + 2], t3 = xi[d + 3] - xj[d + 3];
    s += t0 * t0;
    s += t1 * t1;
    s += t2 * t2;
    s += t3 * t3;
  }
  for (; d < D; ++d) {
    const double t = xi[d] - xj[d];
    s += t * t;
  }
  return s;
}

// gamma = 1 / (2 h^2), h = length_scale, or (length_scale < 0) sqrt(median(sq) / (2 log(n + 1))); h >= 1e-6.
// np.median over all n^2 squared distances: order statistics k1 = (nn - 1) / 2 and k2 = nn / 2 by a radix select on
// the bit patterns (squared distances are >= 0: their bits order like the values), 8 bits per pass from the top, each
// pass recomputing the distances: a 256-bin histogram of the entries that share the prefix found so far, then the bin
// holding rank k1 (thread b owns bin b: a scan over the 256 counts finds it).
__device__ __forceinline__ double svgd_gamma(const double *x, const int n, const int D, const double length_scale,
                                             unsigned *hist_s) {
  const int tid = threadIdx.x;
  const long long nn = (long long)n * n;
  int *scan_s = reinterpret_cast<int *>(hist_s + 256);  // [0..3] wave totals, [4] bin, [5] below
  double h = length_scale;
  if (length_scale < 0.0) {
    const long long k1 = (nn - 1) >> 1, k2 = nn >> 1;
    unsigned long long prefix = 0;
    long long rank = k1;  // rank of the wanted entry among those sharing `prefix`
    for (int shift = 56; shift >= 0; shift -= 8) {
      hist_s[tid] = 0u;
      __syncthreads();
      const unsigned long long hi_mask = shift == 56 ? 0ULL : ~0ULL << (shift + 8);
      for (int e = tid; e < (int)nn; e += BORE_THREADS) {  // (n <= BORE_SVGD_MAX_PARTICLES: n^2 fits 32 bits)
        const int i = e / n, j = e - i * n;
        const unsigned long long v = (unsigned long long)__double_as_longlong(svgd_sqdist(x, D, i, j));
        if ((v & hi_mask) == prefix) atomicAdd(&hist_s[(unsigned)(v >> shift) & 255u], 1u);
      }
      __syncthreads();
      // inclusive scan of the 256 counts: within each wave by shuffles, then the wave totals
      const int cnt = (int)hist_s[tid];
      int incl = cnt;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const int up = __shfl_up(incl, off, 64);
        if ((tid & 63) >= off) incl += up;
      }
      if ((tid & 63) == 63) scan_s[tid >> 6] = incl;
      __syncthreads();
      int base = 0;
      for (int w = 0; w < (tid >> 6); ++w) base += scan_s[w];
      incl += base;
      if (incl - cnt <= rank && rank < incl) {  // exactly one bin holds the rank
        scan_s[4] = tid;
        scan_s[5] = incl - cnt;
      }
      __syncthreads();
      rank -= scan_s[5];
      prefix |= (unsigned long long)scan_s[4] << shift;
      __syncthreads();
    }
    const double v1 = __longlong_as_double((long long)prefix);
    double med = v1;
    if (k2 != k1) {  // even count: the next entry in order = v1 again if it repeats, else min above
      unsigned *cnt_le = hist_s;
      unsigned long long *min_gt = reinterpret_cast<unsigned long long *>(hist_s + 2);
      if (tid == 0) {
        *cnt_le = 0u;
        *min_gt = ~0ULL;
      }
      __syncthreads();
      unsigned c = 0;
      unsigned long long mg = ~0ULL;
      for (int e = tid; e < (int)nn; e += BORE_THREADS) {  // (n <= BORE_SVGD_MAX_PARTICLES: n^2 fits 32 bits)
        const int i = e / n, j = e - i * n;
        const unsigned long long v = (unsigned long long)__double_as_longlong(svgd_sqdist(x, D, i, j));
        if (v <= prefix) ++c;
        else if (v < mg) mg = v;
      }
      atomicAdd(cnt_le, c);
      atomicMin(min_gt, mg);
      __syncthreads();
      const double v2 = (long long)*cnt_le > k2 ? v1 : __longlong_as_double((long long)*min_gt);
      med = (v1 + v2) / 2.0;
      __syncthreads();
    }
    h = sqrt(.5 * med / log((double)(n + 1)));
  }
  h = fmax(h, 1e-6);
  return .5 / (h * h);
}

// zeta = distortion(rank(f)): the constant dparam | (rank / n)^-dparam
__device__ __forceinline__ void svgd_zeta(const double *f, double *zeta, const int n, const int distortion,
                                          const double dparam) {
  for (int i = threadIdx.x; i < n; i += BORE_THREADS) {
    double z = dparam;
    if (distortion == 1) {
      int c = 0;
      for (int j = 0; j < n; ++j) c += f[j] <= f[i];
      z = pow((double)c / (double)n, -dparam);
    }
    zeta[i] = z;
  }
  __syncthreads();
}

// grad_i = (sum_j K_ij zeta_j fg_j + tau 2 sum_j gamma (x_i - x_j) K_ij) / n, K_ij = exp(-gamma |x_i - x_j|^2) formed
// on the fly: a work-item takes particle i and 8 of its coordinates and walks j = 0 .. n-1; the (particle, 8
// coordinates) pairs are dealt over the work-items, particle fastest, in turns beyond BORE_THREADS of them.
__device__ __forceinline__ void svgd_drive_repulsion(const double *x, const double *fg, const double *zeta, double *grad,
                                                     const int n, const int D, const double gamma, const double tau) {
  const int n_work = n * ((D + 7) >> 3);
  for (int w = threadIdx.x; w < n_work; w += BORE_THREADS) {
    const int i = w % n, d0 = 8 * (w / n);
    double drive[8], rep[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) drive[q] = rep[q] = 0.0;
    for (int j = 0; j < n; ++j) {
      const double kij = exp(-gamma * svgd_sqdist(x, D, i, j));
      const double zj = zeta[j];
#pragma unroll
      for (int q = 0; q < 8; ++q)
        if (d0 + q < D) {
          drive[q] += kij * (zj * fg[j * D + d0 + q]);
          rep[q] += gamma * (x[i * D + d0 + q] - x[j * D + d0 + q]) * kij;
        }
    }
#pragma unroll
    for (int q = 0; q < 8; ++q)
      if (d0 + q < D) grad[i * D + d0 + q] = (drive[q] + tau * (2.0 * rep[q])) / (double)n;
  }
  __syncthreads();
}

// Adagrad with momentum -- hist = grad^2 (first iteration) | alpha hist + (1 - alpha) grad^2;
// x += step grad / (eps + sqrt(hist)) -- and the clip into [lo, hi] (the launch's by-value box).
__device__ __forceinline__ void svgd_step_clip(double *x, const double *grad, double *hist, const int nD, const int D,
                                               const bool first, const double step, const double alpha,
                                               const double eps, const int clip, const double *lo, const double *hi) {
  for (int e = threadIdx.x; e < nD; e += BORE_THREADS) {
    const int d = e % D;
    const double g = grad[e];
    const double hs = first ? g * g : alpha * hist[e] + (1.0 - alpha) * (g * g);
    hist[e] = hs;
    double xn = x[e] + step * (g / (eps + sqrt(hs)));
    if (clip) xn = fmin(fmax(xn, lo[d]), hi[d]);
    x[e] = xn;
  }
  __syncthreads();
}

}  // namespace bore
