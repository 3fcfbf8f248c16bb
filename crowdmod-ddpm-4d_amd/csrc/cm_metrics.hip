// The remaining sampling-metric tables of utils/metrics/metricsGenerator.py on the device: SSIM per (sample, channel,
// frame), the mass-conservation energy per sample and the motion-feature histogram metrics (MF_MSE / MF_BHATT).  The
// quantities are the ones crowdmod-ddpm-4d_amd/metrics.py restates on the host (_ssim2d, compute_energy, _mf_polar,
// motion_feature_vectors, bhattacharyya); the arithmetic rules that decide a histogram bin are in include/crowdmod_hip.h.
//
// Every output element has one writer, every floating-point sum has a fixed order (per-thread partial sums over a fixed
// assignment of the work, then a fixed tree over the 256 threads), and the only atomics are integer LDS counters of the
// 2-D histogram counts: two runs give identical bits.
#include <algorithm>
#include <cfloat>
#include <cmath>

#include "cm_kernels.h"

// Nothing in this file may be contracted into a fused multiply-add: the energy residual, the motion-feature scaling and the
// histogram edges are held to the host's operation order bit for bit.
#pragma clang fp contract(off)

namespace cm {

namespace {

// Sum of one value per thread of a 256-thread workgroup in a fixed tree; every thread gets the result.
__device__ __forceinline__ double block_sum256(double v, double *sh) {
  const int tid = threadIdx.x;
  __syncthreads();   // sh may still be read from a previous sum
  sh[tid] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) sh[tid] += sh[tid + s];
    __syncthreads();
  }
  return sh[0];
}

}  // namespace

// --------------------------------------------------------------------------------
// SSIM.  One workgroup per (sample, channel): the [H, W, F] block is contiguous, and is staged band by band (R rows of
// W F floats of both tensors, read with unit stride) into LDS.  A thread owns one frame f = tid % F and every
// (256 / F)-th window of the band; its 49-tap sums and the SSIM value are float64 (the products of two widened float32
// values are exact).  out[n][c][f] = mean over the (H - 6)(W - 6) whole windows.
// --------------------------------------------------------------------------------
struct SsimArgs {
  const float *pred, *gt;
  const double *range;   // [C] data range per channel (device)
  double *out;           // [N][C][F]
  int C, H, W, F, R;     // R: rows of one band (7 <= R <= H)
};

__global__ __launch_bounds__(256) void ssim_frames_kernel(SsimArgs a) {
  extern __shared__ float band[];
  __shared__ double red[256];
  const int tid = threadIdx.x;
  const int H = a.H, W = a.W, F = a.F, WF = W * F, R = a.R, TR = R - 6;
  const int c = blockIdx.x % a.C;
  const size_t base = (size_t)blockIdx.x * H * WF;
  const int nwr = H - 6, nwc = W - 6;
  const int slots = 256 / F, slot = tid / F, f = tid - slot * F;
  float *bp = band, *bg = band + (size_t)R * WF;
  const double Rg = a.range[c];
  const double C1 = (0.01 * Rg) * (0.01 * Rg), C2 = (0.03 * Rg) * (0.03 * Rg);
  const double cov_norm = 49.0 / 48.0;
  double acc = 0.0;
  for (int r0 = 0; r0 < nwr; r0 += TR) {
    const int rows = min(R, H - r0);          // >= 7: r0 < H - 6
    const int cnt = rows * WF;
    __syncthreads();
    for (int i = tid; i < cnt; i += 256) {
      bp[i] = a.pred[base + (size_t)r0 * WF + i];
      bg[i] = a.gt[base + (size_t)r0 * WF + i];
    }
    __syncthreads();
    if (slot < slots) {
      const int nwin = (rows - 6) * nwc;
      for (int w = slot; w < nwin; w += slots) {
        const int i = w / nwc, j = w - i * nwc;
        double sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
        for (int di = 0; di < 7; ++di) {
          const float *px = bp + ((size_t)(i + di) * W + j) * F + f;
          const float *py = bg + ((size_t)(i + di) * W + j) * F + f;
          double rx = 0, ry = 0, rxx = 0, ryy = 0, rxy = 0;
#pragma unroll
          for (int dj = 0; dj < 7; ++dj) {
            const double x = (double)px[dj * F], y = (double)py[dj * F];
            rx += x; ry += y; rxx += x * x; ryy += y * y; rxy += x * y;
          }
          sx += rx; sy += ry; sxx += rxx; syy += ryy; sxy += rxy;
        }
        const double ux = sx / 49.0, uy = sy / 49.0, uxx = sxx / 49.0, uyy = syy / 49.0, uxy = sxy / 49.0;
        const double vx = cov_norm * (uxx - ux * ux), vy = cov_norm * (uyy - uy * uy), vxy = cov_norm * (uxy - ux * uy);
        acc += ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2));
      }
    }
  }
  red[tid] = acc;
  __syncthreads();
  if (tid < F) {
    double s = 0.0;
    for (int k = 0; k < slots; ++k) s += red[k * F + tid];
    a.out[(size_t)blockIdx.x * F + tid] = s / ((double)nwr * (double)nwc);
  }
}

bool ssim_frames_ok(int W, int F) { return (long long)W * F <= kSsimMaxRow; }

hipError_t launch_ssim_frames(const float *pred, const float *gt, int N, int C, int H, int W, int F, const double *range,
                              double *out, hipStream_t st) {
  if (N < 1 || C < 1 || F < 1 || H < 7 || W < 7 || !ssim_frames_ok(W, F) || (long long)N * C > 0x7fffffffLL) return hipErrorInvalidValue;
  const int WF = W * F;
  const int R = std::max(7, std::min(H, kSsimBandFloats / (2 * WF)));   // kSsimMaxRow * 14 <= kSsimBandFloats
  SsimArgs a{pred, gt, range, out, C, H, W, F, R};
  hipLaunchKernelGGL(ssim_frames_kernel, dim3(N * C), dim3(256), (size_t)2 * R * WF * sizeof(float), st, a);
  return hipGetLastError();
}

// --------------------------------------------------------------------------------
// Energy (models/guidance.py:10-42): one workgroup per sample.  The residual of an interior cell is float32 in the host's
// operation order; its square and the sum are float64.
// --------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void energy_kernel(const float *__restrict__ x, int C, int H, int W, int L, float it,
                                                     float il, float f0, float f1, float f2, double *__restrict__ out) {
  __shared__ double red[256];
  const size_t HWL = (size_t)H * W * L;
  const float *r = x + (size_t)blockIdx.x * C * HWL, *u = r + HWL, *v = u + HWL;
  const long long nl = L - 1, nw = W - 2, nh = H - 2;
  const long long ncell = (nl > 0 && nw > 0 && nh > 0) ? nl * nw * nh : 0;
  const size_t sh = (size_t)W * L, sw = (size_t)L;
  double acc = 0.0;
  for (long long e = threadIdx.x; e < ncell; e += 256) {
    const long long l = e % nl, q = e / nl;
    const long long w = 1 + q % nw, h = 1 + q / nw;
    const size_t o = ((size_t)h * W + w) * L + l;
    const float rr = r[o] * f0, uu = u[o] * f1, vv = v[o] * f2;
    const float t1 = it * (r[o + 1] * f0 - rr);
    const float t2 = (il * rr) * ((u[o + sh] * f1 - uu) + (v[o + sw] * f2 - vv));
    const float t3 = (il * (r[o + sh] * f0 - rr)) * uu;
    const float t4 = (il * (r[o + sw] * f0 - rr)) * vv;
    const float f = ((t1 + t2) + t3) + t4;
    acc += (double)f * (double)f;
  }
  const double s = block_sum256(acc, red);
  if (threadIdx.x == 0) out[blockIdx.x] = (0.5 * s) / ((double)H * (double)W * (double)L);
}

hipError_t launch_energy(const float *x, int N, int C, int H, int W, int L, float inv_dt, float inv_dl, const float fac[3],
                         double *out, hipStream_t st) {
  if (N < 1 || C < 3 || H < 1 || W < 1 || L < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(energy_kernel, dim3(N), dim3(256), 0, st, x, C, H, W, L, inv_dt, inv_dl, fac[0], fac[1], fac[2], out);
  return hipGetLastError();
}

// --------------------------------------------------------------------------------
// Motion features (utils/metrics/motionFeatureExtractor.py:34-59,166-303).
// --------------------------------------------------------------------------------
namespace {

struct MfElem {
  int bin2;    // index in the volume's 16 x 16 count histogram (first magnitude bin already moved to angle bin 8); -1: outside
  int ab1;     // angle bin of the 1-D histogram; -1: outside
  double wt;   // log-magnitude ** gamma
};

// One element (frame t of the grid cell whose F frames start at vx / vy).  The rules are those of the header comment over
// cm_motion_feature_vectors.
__device__ MfElem mf_element(const float *__restrict__ vx, const float *__restrict__ vy, int F, int t, double gamma) {
  double lo = INFINITY, hi = -INFINITY, mag = 0.0;
  bool nan = false;
  float xt = 0.f, yt = 0.f;
  for (int j = 0; j < F; ++j) {
    const float x = vx[j], y = vy[j];
    const float px = x * x, py = y * y;
    const float m = sqrtf(px + py);           // float32, every step rounded; the square root is correctly rounded
    const double md = (double)m;
    nan |= (m != m);
    lo = fmin(lo, md);
    hi = fmax(hi, md);
    if (j == t) { mag = md; xt = x; yt = y; }
  }
  if (nan) lo = hi = (double)NAN;             // numpy's min / max propagate a NaN to the whole cell
  double rng = hi - lo;
  if (rng < 10.0 * DBL_EPSILON) rng = 1.0;
  const double scale = 255.0 / rng;
  const double y = (mag * scale + (0.0 - lo * scale)) + 1.0;
  const double lm = (y == 1.0) ? 0.0 : log2(y);
  // magnitude bin: edges i / 2 on lm; the top edge is decided on y itself (256 + 2 ulp still rounds to log2 = 8)
  int mb = -1;
  if (y >= 256.0) {
    if (y <= 256.0 + 2.0 * 0x1p-44) mb = 15;
  } else if (lm >= 0.0) {
    mb = min(15, (int)floor(lm * 2.0));
  }
  // angle: float32 atan2 widened; the exact cases are pinned (a zero v_y with negative v_x is +-pi in float32)
  float af;
  if (yt == 0.f && xt < 0.f) af = copysignf(3.14159274101257324f, yt);
  else af = atan2f(yt, xt);
  const double ang = (double)af;
  const double pi = 3.141592653589793, step = pi / 8.0;
  int ab = -1;                                // searchsorted(edges, ang, side='right') - 1, edges = linspace(-pi, pi, 17)
  for (int i = 0; i < 17; ++i) {
    const double edge = i == 16 ? pi : (double)i * step + (-pi);
    if (edge <= ang) ab = i;
  }
  const int ab2 = (ang == pi) ? 15 : ab;      // histogram2d closes its last bin; digitize (the 1-D one) does not
  MfElem el;
  el.bin2 = (mb >= 0 && ab2 >= 0 && ab2 < 16) ? (mb == 0 ? 8 : mb * 16 + ab2) : -1;
  el.ab1 = (ab >= 0 && ab < 16) ? ab : -1;
  el.wt = pow(lm, gamma);
  return el;
}

struct MfArgs {
  const float *a, *b;     // [N][C][H][W][F]; vectors: a only
  int C, H, W, F, f, k, nvr, nvc, nvol;
  double gamma;
  double *mf2, *mf1;      // vectors: [N][nvol * 256], [N][nvol * 16]
  double *out;            // tables: [N][6]
};

}  // namespace

// One workgroup per sample.  Pass 1 (all 256 threads over the sample's elements): the normalisers, count + 1 and weight
// sum + 1.  Pass 2: one wave per volume (f x k x k elements): counts into its own LDS histogram, the 16 weighted angle sums
// in lanes 0-15 (elements visited in index order through lane broadcasts), then either the normalised vectors are
// written (TABLES = false) or the per-bin differences / geometric means of the two sequences are accumulated.
template <bool TABLES>
__global__ __launch_bounds__(256) void motion_feature_kernel(MfArgs a) {
  constexpr int NT = TABLES ? 2 : 1;
  __shared__ double red[256];
  __shared__ int h2[4][NT][256];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int H = a.H, W = a.W, F = a.F;
  const size_t HWF = (size_t)H * W * F;
  const float *seq[NT];
  seq[0] = a.a + (size_t)blockIdx.x * a.C * HWF;
  if (TABLES) seq[NT - 1] = a.b + (size_t)blockIdx.x * a.C * HWF;
  double tot2[NT], tot1[NT];
  for (int s = 0; s < NT; ++s) {
    const float *vx = seq[s] + HWF, *vy = seq[s] + 2 * HWF;
    double cnt = 0.0, sw = 0.0;
    for (size_t e = tid; e < HWF; e += 256) {
      const size_t cell = e / F;
      const MfElem el = mf_element(vx + cell * F, vy + cell * F, F, (int)(e - cell * F), a.gamma);
      if (el.bin2 >= 0) cnt += 1.0;
      if (el.ab1 >= 0) sw += el.wt;
    }
    tot2[s] = block_sum256(cnt, red) + 1.0;
    tot1[s] = block_sum256(sw, red) + 1.0;
  }
  double mse2 = 0, bc2 = 0, mse1 = 0, bc1 = 0;
  for (int v0 = 0; v0 < a.nvol; v0 += 4) {
    const int v = v0 + wave;
    const bool valid = v < a.nvol;
    __syncthreads();                          // the previous round's histograms have been consumed
    for (int s = 0; s < NT; ++s)
      for (int b = lane; b < 256; b += 64) h2[wave][s][b] = 0;
    __syncthreads();
    double w1[NT];
    for (int s = 0; s < NT; ++s) w1[s] = 0.0;
    if (valid) {
      const int cb = v % a.nvc, rb = (v / a.nvc) % a.nvr, fb = v / (a.nvc * a.nvr);
      const int t0 = fb * a.f, r0 = rb * a.k, c0 = cb * a.k;
      const int nf = min(a.f, F - t0), nr = min(a.k, H - r0), ncol = min(a.k, W - c0);
      const int nel = nf * nr * ncol;         // <= f k k, checked by the launcher to fit an int
      for (int s = 0; s < NT; ++s) {
        const float *vx = seq[s] + HWF, *vy = seq[s] + 2 * HWF;
        for (int e0 = 0; e0 < nel; e0 += 64) {
          const int e = e0 + lane;
          MfElem el;
          el.bin2 = -1; el.ab1 = -1; el.wt = 0.0;
          if (e < nel) {
            const int tt = e % nf, q = e / nf;
            const int cc = q % ncol, rr = q / ncol;
            const size_t cell = (size_t)(r0 + rr) * W + (c0 + cc);
            el = mf_element(vx + cell * F, vy + cell * F, F, t0 + tt, a.gamma);
            if (el.bin2 >= 0) atomicAdd(&h2[wave][s][el.bin2], 1);
          }
          const int m = min(64, nel - e0);
          for (int j = 0; j < m; ++j) {
            const int abj = __shfl(el.ab1, j);
            const double wj = __shfl(el.wt, j);
            if (abj == lane) w1[s] += wj;
          }
        }
      }
    }
    __syncthreads();
    if (valid) {
      if (TABLES) {
        for (int b = lane; b < 256; b += 64) {
          const double p = (double)h2[wave][0][b] / tot2[0], g = (double)h2[wave][NT - 1][b] / tot2[NT - 1];
          const double d = g - p;
          mse2 += d * d;
          bc2 += sqrt(g * p);
        }
        if (lane < 16) {
          const double p = w1[0] / tot1[0], g = w1[NT - 1] / tot1[NT - 1];
          const double d = g - p;
          mse1 += d * d;
          bc1 += sqrt(g * p);
        }
      } else {
        double *o2 = a.mf2 + ((size_t)blockIdx.x * a.nvol + v) * 256;
        for (int b = lane; b < 256; b += 64) o2[b] = (double)h2[wave][0][b] / tot2[0];
        if (lane < 16) a.mf1[((size_t)blockIdx.x * a.nvol + v) * 16 + lane] = w1[0] / tot1[0];
      }
    }
  }
  if (TABLES) {
    const double m2 = block_sum256(mse2, red), c2 = block_sum256(bc2, red);
    const double m1 = block_sum256(mse1, red), c1 = block_sum256(bc1, red);
    if (tid == 0) {
      double *o = a.out + (size_t)blockIdx.x * 6;
      const double k2 = c2 != c2 ? c2 : fmin(fmax(c2, 0.01), 1.0);   // np.clip keeps a NaN
      const double k1 = c1 != c1 ? c1 : fmin(fmax(c1, 0.01), 1.0);
      o[0] = m2 / ((double)a.nvol * 256.0);
      o[1] = m1 / ((double)a.nvol * 16.0);
      o[2] = -log(k2);
      o[3] = -log(k1);
      o[4] = k2;
      o[5] = k1;
    }
  }
}

long long motion_feature_volumes(int H, int W, int F, int f, int k) {
  const long long nvf = ((long long)F + f - 1) / f, nvr = ((long long)H + k - 1) / k, nvc = ((long long)W + k - 1) / k;
  return nvf * nvr * nvc;
}

hipError_t launch_motion_features(const float *a, const float *b, int N, int C, int H, int W, int F, int f, int k, double gamma,
                                  double *mf2, double *mf1, double *out, hipStream_t st) {
  if (N < 1 || C < 3 || H < 1 || W < 1 || F < 1 || f < 1 || k < 1 || !a) return hipErrorInvalidValue;
  f = std::min(f, F);                         // a larger block is one ragged block: the same volumes
  k = std::min(k, std::max(H, W));
  const long long nvol = motion_feature_volumes(H, W, F, f, k);
  if (nvol > 0x7fffffffLL || (long long)f * k * k > 0x7fffffffLL) return hipErrorInvalidValue;
  MfArgs g{a, b, C, H, W, F, f, k, (H + k - 1) / k, (W + k - 1) / k, (int)nvol, gamma, mf2, mf1, out};
  if (b) {
    if (!out) return hipErrorInvalidValue;
    hipLaunchKernelGGL(motion_feature_kernel<true>, dim3(N), dim3(256), 0, st, g);
  } else {
    if (!mf2 || !mf1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(motion_feature_kernel<false>, dim3(N), dim3(256), 0, st, g);
  }
  return hipGetLastError();
}

}  // namespace cm
