// ConvRNN training kernels (reference: models/convRNN/convRNN.py:98-171, utils/loss.py:15-52).  The host plan lives in
// cm_convrnn_train_host.inc; the training forward is cm_convrnn.hip's crnn_conv_kernel writing into tape slots.
//
//   crnn_dgrad_kernel  data gradient of a conv as a gather-form implicit GEMM on v_mfma_f32_32x32x2_f32 (exact fp32 products),
//                      the forward's 64 x 64 x 32 tile: M = destination pixels of all samples, N = the conv's input channels
//                      (both sources of a cell's [x, h]), K = taps * output channels.  3x3 stride 1: the same geometry on
//                      transposed, flipped weights; 3x3 stride 2: four output-parity classes of 1 / 2 / 2 / 4 taps;
//                      ConvTranspose2d 4x4 stride 2: a 4x4 stride-2 pad-1 conv of 16 taps.  Never a scatter.
//   crnn_wgrad_kernel  dW[n][tap][c] = sum over (b, pixel) of dy[n] x_shifted[c]: M = output channels, N = taps * input
//                      channels, K = pixels of all samples, split in ranges; a workgroup ADDS its tile to the partial of its
//                      range (one writer per element; the applications of a weight are launches in stream order), and
//                      crnn_wgrad_reduce_kernel sums the ranges in order into the reference layout.
//   gate backward, loss (float64 partials, fixed-order finalise), d loss / d yhat: elementwise (the AMSGrad update is cm_train.hip's launch_adam).
// Every global address is guarded: rows by the pixel count, columns by the channel count, taps by the source grid.
#include "cm_kernels.h"

#include <math.h>

namespace cm {

typedef float crnnt_f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int TB = 64, TK = 32, TS = TK + 1, CS = TB + 1;   // as in cm_convrnn.hip

// source pixel of tap `tap` seen from row pixel (qy, qx); false outside the source grid
template <int GEO>
__device__ __forceinline__ bool bg_src(int tap, int qy, int qx, int py, int px, int Hs, int Ws, int *iy, int *ix) {
  if (GEO == CRNN_BG_S1) { *iy = qy + tap / 3 - 1; *ix = qx + tap % 3 - 1; }
  else if (GEO == CRNN_BG_S2) { *iy = 2 * qy + tap / 3 - 1; *ix = 2 * qx + tap % 3 - 1; }
  else if (GEO == CRNN_BG_G4) { *iy = 2 * qy - 1 + (tap >> 2); *ix = 2 * qx - 1 + (tap & 3); }
  else { *iy = qy + py - tap / (1 + px); *ix = qx + px - tap % (1 + px); }
  return *iy >= 0 && *iy < Hs && *ix >= 0 && *ix < Ws;
}

template <int GEO>
__global__ __launch_bounds__(256) void crnn_dgrad_kernel(const CrnnDgradArgs a) {
  __shared__ float S[2 * TB * TS];
  float *As = S, *Ws = S + TB * TS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cls = GEO == CRNN_BG_P3 ? (int)blockIdx.z : 0, py = cls >> 1, px = cls & 1;
  const int Hm = GEO == CRNN_BG_P3 ? a.Hs : a.Hd, Wm = GEO == CRNN_BG_P3 ? a.Ws : a.Wd_;
  const int M = a.B * Hm * Wm, N = a.C0 + a.C1;
  const int m0 = blockIdx.x * TB, n0 = blockIdx.y * TB;
  const int ntaps = GEO == CRNN_BG_G4 ? 16 : GEO == CRNN_BG_P3 ? (1 + py) * (1 + px) : 9;
  const int K = ntaps * a.Cs;
  const int before = cls == 0 ? 0 : cls == 1 ? 1 : cls == 2 ? 3 : 5;   // taps of the classes in front of this one
  const float *W = a.Wd + (long long)before * N * a.Cs;

  crnnt_f32x16 acc;
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  const int wm = wave & 1, wn = wave >> 1;
  const int sr = tid >> 2, sk = (tid & 3) * 8;
  const int r = m0 + sr, n = n0 + sr;
  const bool rok = r < M;
  const int b = rok ? r / (Hm * Wm) : 0, q = rok ? r % (Hm * Wm) : 0, qy = q / Wm, qx = q % Wm;
  const float *s0 = a.dy + (long long)b * a.Hs * a.Ws * a.Cs;
  for (int k0 = 0; k0 < K; k0 += TK) {
    const int k = k0 + sk;
    float4 v0 = make_float4(0.f, 0.f, 0.f, 0.f), v1 = v0, w0 = v0, w1 = v0;
    if (k < K) {
      const int tap = k / a.Cs, c = k - tap * a.Cs;
      int iy, ix;
      if (bg_src<GEO>(tap, qy, qx, py, px, a.Hs, a.Ws, &iy, &ix) && rok) {
        const float *p = s0 + ((long long)iy * a.Ws + ix) * a.Cs + c;
        v0 = *(const float4 *)p; v1 = *(const float4 *)(p + 4);
      }
      if (n < N) {
        const float *p = W + (long long)n * K + k;
        w0 = *(const float4 *)p; w1 = *(const float4 *)(p + 4);
      }
    }
    float *ad = As + sr * TS + sk, *wd = Ws + sr * TS + sk;
    ad[0] = v0.x; ad[1] = v0.y; ad[2] = v0.z; ad[3] = v0.w; ad[4] = v1.x; ad[5] = v1.y; ad[6] = v1.z; ad[7] = v1.w;
    wd[0] = w0.x; wd[1] = w0.y; wd[2] = w0.z; wd[3] = w0.w; wd[4] = w1.x; wd[5] = w1.y; wd[6] = w1.z; wd[7] = w1.w;
    __syncthreads();
    const float *ap = As + (wm * 32 + (lane & 31)) * TS + (lane >> 5);
    const float *bp = Ws + (wn * 32 + (lane & 31)) * TS + (lane >> 5);
    crnnt_f32x16 part;
#pragma unroll
    for (int i = 0; i < 16; ++i) part[i] = 0.f;
#pragma unroll
    for (int kk = 0; kk < TK; kk += 2) part = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[kk], bp[kk], part, 0, 0, 0);
    acc += part;
    __syncthreads();
  }

  float *Cs = S;
#pragma unroll
  for (int i = 0; i < 16; ++i)
    Cs[(wm * 32 + (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5)) * CS + wn * 32 + (lane & 31)] = acc[i];
  __syncthreads();

  for (int e = tid; e < TB * TB; e += 256) {
    const int row = e / TB, cl = e % TB;
    const int rl = m0 + row, col = n0 + cl;
    if (rl >= M || col >= N) continue;
    const int eb = rl / (Hm * Wm), eq = rl % (Hm * Wm);
    const int oy = GEO == CRNN_BG_P3 ? 2 * (eq / Wm) + py : eq / Wm, ox = GEO == CRNN_BG_P3 ? 2 * (eq % Wm) + px : eq % Wm;
    const long long ip = (long long)oy * a.Wd_ + ox, pix = (long long)eb * a.Hd * a.Wd_ + ip;
    const float v = Cs[row * CS + cl];
    if (col < a.C0) {
      if (!a.d0) continue;
      if (a.fb_exp) {
        if (col >= a.fb_C) continue;
        const float f = (col == 0 || col == 3) ? a.fb_exp[(long long)eb * a.fb_bs + ip * 8 + col] : 1.0f;
        a.d0[pix * 8 + col] += v * f;
        continue;
      }
      const long long o = pix * a.C0 + col;
      float val = a.acc0 ? a.d0[o] + v : v;
      if (a.mask0) val *= a.mask0[o] > 0.f ? 1.0f : 0.2f;
      a.d0[o] = val;
    } else {
      const int ch = col - a.C0;
      const long long o = pix * a.C1 + ch;
      if (a.gr) {
        const float rr = a.gr[o];
        a.d1[o] += v * rr;
        a.gdr[pix * 2 * a.C1 + ch] = v * a.gh[o] * rr * (1.0f - rr);
      } else {
        a.d1[o] = a.acc1 ? a.d1[o] + v : v;
      }
    }
  }
}

template <int GEO>
__global__ __launch_bounds__(256) void crnn_wgrad_kernel(const CrnnWgradArgs a) {
  __shared__ float S[2 * TB * TS];
  float *As = S, *Ws = S + TB * TS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int M = a.B * a.Hm * a.Wm, Cin = a.C0 + a.C1;
  const int ntaps = GEO == CRNN_BG_G4 ? 16 : 9, Kt = ntaps * Cin;
  const int k0c = blockIdx.x * TB, n0 = blockIdx.y * TB;
  const int per = ((M + a.nsplit - 1) / a.nsplit + TK - 1) / TK * TK;
  const int mb = (int)blockIdx.z * per, me = min(M, mb + per);

  crnnt_f32x16 acc;
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  const int wm = wave & 1, wn = wave >> 1;
  const int ml = tid >> 3, j8 = (tid & 7) * 8;   // staging: one row pixel, eight consecutive columns of each operand
  const int nn = n0 + j8, kc = k0c + j8;
  const bool kok = kc < Kt;
  const int tap = kok ? kc / Cin : 0, c = kc - tap * Cin;
  for (int mm = mb; mm < me; mm += TK) {
    const int m = mm + ml;
    float4 v0 = make_float4(0.f, 0.f, 0.f, 0.f), v1 = v0, w0 = v0, w1 = v0;
    if (m < me) {
      const int b = m / (a.Hm * a.Wm), q = m % (a.Hm * a.Wm), qy = q / a.Wm, qx = q % a.Wm;
      if (nn < a.Nr) {
        const float *p = a.R + (long long)m * a.Nr + nn;
        v0 = *(const float4 *)p; v1 = *(const float4 *)(p + 4);
      }
      int iy, ix;
      if (kok && bg_src<GEO>(tap, qy, qx, 0, 0, a.Hs, a.Ws, &iy, &ix)) {
        const long long pix = (long long)iy * a.Ws + ix;
        const float *p = c < a.C0 ? a.x0 + (long long)b * a.bs0 + pix * a.C0 + c : a.x1 + (long long)b * a.bs1 + pix * a.C1 + (c - a.C0);
        w0 = *(const float4 *)p; w1 = *(const float4 *)(p + 4);
      }
    }
    float *ad = As + j8 * TS + ml, *wd = Ws + j8 * TS + ml;
    ad[0] = v0.x; ad[TS] = v0.y; ad[2 * TS] = v0.z; ad[3 * TS] = v0.w; ad[4 * TS] = v1.x; ad[5 * TS] = v1.y; ad[6 * TS] = v1.z; ad[7 * TS] = v1.w;
    wd[0] = w0.x; wd[TS] = w0.y; wd[2 * TS] = w0.z; wd[3 * TS] = w0.w; wd[4 * TS] = w1.x; wd[5 * TS] = w1.y; wd[6 * TS] = w1.z; wd[7 * TS] = w1.w;
    __syncthreads();
    const float *ap = As + (wm * 32 + (lane & 31)) * TS + (lane >> 5);
    const float *bp = Ws + (wn * 32 + (lane & 31)) * TS + (lane >> 5);
    crnnt_f32x16 part;
#pragma unroll
    for (int i = 0; i < 16; ++i) part[i] = 0.f;
#pragma unroll
    for (int kk = 0; kk < TK; kk += 2) part = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[kk], bp[kk], part, 0, 0, 0);
    acc += part;
    __syncthreads();
  }
  // C/D map: column = lane & 31, row = (i & 3) + 8 (i >> 2) + 4 (lane >> 5)
  float *P = a.part + (long long)blockIdx.z * a.Nr * Kt;
  const int col = k0c + wn * 32 + (lane & 31);
  if (col >= Kt) return;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int row = n0 + wm * 32 + (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
    if (row < a.Nr) P[(long long)row * Kt + col] += acc[i];
  }
}

__global__ __launch_bounds__(256) void crnn_wgrad_reduce_kernel(const float *part, int nsplit, long long zstride, long long n, const unsigned *idx,
                                                                float *grad) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n || !idx[e]) return;
  float s = part[e];
  for (int z = 1; z < nsplit; ++z) s += part[(long long)z * zstride + e];
  grad[idx[e] - 1] = s;
}

__global__ __launch_bounds__(256) void crnn_gather_kernel(const float *master, const unsigned *idx, float *dst, long long n) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  dst[e] = idx[e] ? master[idx[e] - 1] : 0.f;
}

__global__ __launch_bounds__(256) void crnn_gru_bwd_kernel(const float *dcur, const float *u, const float *cand, const float *hprev,
                                                           float *dprev, float *dcand, float *dru, long long n, int hid) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float d = dcur[i], uu = u[i], cc = cand[i];
  dprev[i] = d * uu;
  dcand[i] = d * (1.0f - uu) * (1.0f - cc * cc);
  dru[(i / hid) * 2 * hid + hid + i % hid] = d * (hprev[i] - cc) * uu * (1.0f - uu);
}

__global__ __launch_bounds__(256) void crnn_lstm_bwd_kernel(const float *dcur, const float *gates, const float *cprev, const float *tc,
                                                            float *dc, float *dprev, float *dpre, long long n) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float4 g = *(const float4 *)(gates + 4 * i);   // i, f, o, g
  const float d = dcur[i], t = tc[i];
  const float dct = dc[i] + d * g.z * (1.0f - t * t);
  dc[i] = dct * g.y;
  dprev[i] = 0.f;
  *(float4 *)(dpre + 4 * i) = make_float4(dct * g.w * g.x * (1.0f - g.x), dct * cprev[i] * g.y * (1.0f - g.y),
                                          d * t * g.z * (1.0f - g.z), dct * g.x * (1.0f - g.w * g.w));
}

__global__ __launch_bounds__(256) void crnn_add_kernel(float *dst, const float *src, long long n) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) dst[i] += src[i];
}

// the clamped exp of utils/loss.py:19,31 and whether the clamp passes gradient ([min, max] inclusive)
__device__ __forceinline__ double clamp_exp(float v, bool *pass) {
  const double e = exp((double)v);
  *pass = e >= 1e-8 && e <= 20.0;
  return e < 1e-8 ? 1e-8 : e > 20.0 ? 20.0 : e;
}
__device__ __forceinline__ double clamp_gt(float v) { return v < 1e-8f ? (double)1e-8f : v > 20.f ? 20.0 : (double)v; }

__global__ __launch_bounds__(256) void crnn_loss_partial_kernel(const float *yhat, const float *y, long long n, int HW, int F, double *part) {
  __shared__ double R[5][256];
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  double s[5] = {0, 0, 0, 0, 0};
  if (i < n) {
    const long long per = (long long)HW * F, b = i / per, o = b * 4 * per + i % per;
    bool pass;
    const double rho_hat = clamp_exp(yhat[o], &pass), rho_gt = clamp_gt(y[o]);
    const double var_hat = clamp_exp(yhat[o + 3 * per], &pass), var_gt = clamp_gt(y[o + 3 * per]);
    const double m1 = yhat[o + per], m2 = yhat[o + 2 * per], e1 = m1 - (double)y[o + per], e2 = m2 - (double)y[o + 2 * per];
    s[0] = rho_gt * (log(rho_gt) - log(rho_hat)) + rho_hat - rho_gt;
    if (rho_gt >= 1.0) { s[1] = e1 * e1 + e2 * e2 + 2.0 * (var_hat - var_gt) * (var_hat - var_gt); s[2] = 1.0; }
    else { s[3] = m1 * m1 + m2 * m2 + var_hat * var_hat; s[4] = 1.0; }
  }
  for (int j = 0; j < 5; ++j) R[j][threadIdx.x] = s[j];
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w)
      for (int j = 0; j < 5; ++j) R[j][threadIdx.x] += R[j][threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x < 5) part[(long long)blockIdx.x * 5 + threadIdx.x] = R[threadIdx.x][0];
}

__global__ void crnn_loss_final_kernel(const double *part, int nblocks, double n, double eps, double *sums, double *terms) {
  __shared__ double s[5];
  if (threadIdx.x < 5) {
    double t = 0;
    for (int k = 0; k < nblocks; ++k) t += part[(long long)k * 5 + threadIdx.x];
    s[threadIdx.x] = sums[threadIdx.x] = t;
  }
  __syncthreads();
  if (threadIdx.x == 0 && terms) crnn_loss_terms(s, n, eps, terms);
}

__global__ void crnn_loss_terms_kernel(const double *sums6, double eps, double *terms) {
  if (threadIdx.x == 0 && blockIdx.x == 0) crnn_loss_terms(sums6, sums6[5], eps, terms);
}

__global__ __launch_bounds__(256) void crnn_loss_grad_kernel(const float *yhat, const float *y, long long n, int B, int HW, int F, double eps,
                                                             double alpha, const double *sums, double n_den, float *dY) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long long per = (long long)HW * F, b = i / per, rem = i % per, o = b * 4 * per + rem;
  const int p = (int)(rem / F), t = (int)(rem % F);
  bool pr, pv;
  const double rho_hat = clamp_exp(yhat[o], &pr), rho_gt = clamp_gt(y[o]);
  const double var_hat = clamp_exp(yhat[o + 3 * per], &pv), var_gt = clamp_gt(y[o + 3 * per]);
  const double m1 = yhat[o + per], m2 = yhat[o + 2 * per];
  const double g0 = pr ? (1.0 - rho_gt / rho_hat) / n_den * rho_hat : 0.0;
  double g1, g2, g3;
  if (rho_gt >= 1.0) {
    const double w = alpha / crnn_loss_den(sums[2], eps);
    g1 = 2.0 * (m1 - (double)y[o + per]) * w; g2 = 2.0 * (m2 - (double)y[o + 2 * per]) * w; g3 = 4.0 * (var_hat - var_gt) * w;
  } else {
    const double w = alpha / crnn_loss_den(sums[4], eps);
    g1 = 2.0 * m1 * w; g2 = 2.0 * m2 * w; g3 = 2.0 * var_hat * w;
  }
  g3 = pv ? g3 * var_hat : 0.0;
  float4 *d = (float4 *)(dY + (((long long)t * B + b) * HW + p) * 8);
  d[0] = make_float4((float)g0, (float)g1, (float)g2, (float)g3);
  d[1] = make_float4(0.f, 0.f, 0.f, 0.f);
}

inline unsigned blocks_of(long long n) { return (unsigned)((n + 255) / 256); }

}  // namespace

hipError_t launch_crnn_dgrad(const CrnnDgradArgs &a, hipStream_t st) {
  const bool p3 = a.geo == CRNN_BG_P3;
  const long long M = (long long)a.B * (p3 ? a.Hs : a.Hd) * (p3 ? a.Ws : a.Wd_);
  const int N = a.C0 + a.C1;
  if (M <= 0) return hipSuccess;
  if (M > 0x7fffffffLL - TB || a.Cs < 8 || a.Cs % 8 || a.C0 < 1 || a.C1 < 0 || !a.dy || !a.Wd || (a.C1 > 0 && !a.d1)) return hipErrorInvalidValue;
  if (a.geo == CRNN_BG_S1 ? (a.Hs != a.Hd || a.Ws != a.Wd_) : a.geo == CRNN_BG_G4 ? (a.Hs != 2 * a.Hd || a.Ws != 2 * a.Wd_)
                                                            : p3 ? (a.Hd != 2 * a.Hs || a.Wd_ != 2 * a.Ws) : true)
    return hipErrorInvalidValue;
  if (a.gr && (!a.gh || !a.gdr)) return hipErrorInvalidValue;
  if (a.fb_exp && (!a.d0 || a.fb_C > 8 || a.fb_C > a.C0)) return hipErrorInvalidValue;
  dim3 grid((unsigned)((M + TB - 1) / TB), (unsigned)((N + TB - 1) / TB), p3 ? 4 : 1);
  if (a.geo == CRNN_BG_S1) hipLaunchKernelGGL((crnn_dgrad_kernel<CRNN_BG_S1>), grid, dim3(256), 0, st, a);
  else if (a.geo == CRNN_BG_G4) hipLaunchKernelGGL((crnn_dgrad_kernel<CRNN_BG_G4>), grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL((crnn_dgrad_kernel<CRNN_BG_P3>), grid, dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_crnn_wgrad(const CrnnWgradArgs &a, hipStream_t st) {
  const long long M = (long long)a.B * a.Hm * a.Wm;
  if (M <= 0) return hipSuccess;
  if (M > 0x7fffffffLL - TB * 64 || a.Nr < 8 || a.Nr % 8 || a.C0 < 8 || a.C0 % 8 || a.C1 < 0 || a.C1 % 8 || (a.C1 > 0) != (a.x1 != nullptr) ||
      a.nsplit < 1 || a.nsplit > 64 || !a.R || !a.x0 || !a.part)
    return hipErrorInvalidValue;
  if (a.geo == CRNN_BG_S1 ? (a.Hs != a.Hm || a.Ws != a.Wm) : (a.geo == CRNN_BG_S2 || a.geo == CRNN_BG_G4) ? (a.Hs != 2 * a.Hm || a.Ws != 2 * a.Wm) : true)
    return hipErrorInvalidValue;
  const int Kt = (a.geo == CRNN_BG_G4 ? 16 : 9) * (a.C0 + a.C1);
  dim3 grid((unsigned)((Kt + TB - 1) / TB), (unsigned)((a.Nr + TB - 1) / TB), (unsigned)a.nsplit);
  if (a.geo == CRNN_BG_S1) hipLaunchKernelGGL((crnn_wgrad_kernel<CRNN_BG_S1>), grid, dim3(256), 0, st, a);
  else if (a.geo == CRNN_BG_S2) hipLaunchKernelGGL((crnn_wgrad_kernel<CRNN_BG_S2>), grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL((crnn_wgrad_kernel<CRNN_BG_G4>), grid, dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_crnn_wgrad_reduce(const float *part, int nsplit, long long zstride, long long n, const unsigned *idx, float *grad,
                                    hipStream_t st) {
  if (n <= 0) return hipSuccess;
  if (n > zstride || nsplit < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(crnn_wgrad_reduce_kernel, dim3(blocks_of(n)), dim3(256), 0, st, part, nsplit, zstride, n, idx, grad);
  return hipGetLastError();
}

hipError_t launch_crnn_gather(const float *master, const unsigned *idx, float *dst, long long n, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(crnn_gather_kernel, dim3(blocks_of(n)), dim3(256), 0, st, master, idx, dst, n);
  return hipGetLastError();
}

hipError_t launch_crnn_gru_bwd(const float *dcur, const float *u, const float *cand, const float *hprev, float *dprev, float *dcand,
                               float *dru, long long n, int hid, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(crnn_gru_bwd_kernel, dim3(blocks_of(n)), dim3(256), 0, st, dcur, u, cand, hprev, dprev, dcand, dru, n, hid);
  return hipGetLastError();
}

hipError_t launch_crnn_lstm_bwd(const float *dcur, const float *gates, const float *cprev, const float *tc, float *dc, float *dprev,
                                float *dpre, long long n, int hid, hipStream_t st) {
  (void)hid;
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(crnn_lstm_bwd_kernel, dim3(blocks_of(n)), dim3(256), 0, st, dcur, gates, cprev, tc, dc, dprev, dpre, n);
  return hipGetLastError();
}

hipError_t launch_crnn_add(float *dst, const float *src, long long n, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(crnn_add_kernel, dim3(blocks_of(n)), dim3(256), 0, st, dst, src, n);
  return hipGetLastError();
}

hipError_t launch_crnn_loss(const float *yhat, const float *y, int B, int HW, int F, double eps, double *part, double *sums, double *terms,
                            hipStream_t st) {
  const long long n = (long long)B * HW * F;
  if (n <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(crnn_loss_partial_kernel, dim3(blocks_of(n)), dim3(256), 0, st, yhat, y, n, HW, F, part);
  hipLaunchKernelGGL(crnn_loss_final_kernel, dim3(1), dim3(64), 0, st, part, (int)blocks_of(n), (double)n, eps, sums, terms);
  return hipGetLastError();
}

hipError_t launch_crnn_loss_terms(const double *sums6, double eps, double *terms, hipStream_t st) {
  hipLaunchKernelGGL(crnn_loss_terms_kernel, dim3(1), dim3(64), 0, st, sums6, eps, terms);
  return hipGetLastError();
}

hipError_t launch_crnn_loss_grad(const float *yhat, const float *y, int B, int HW, int F, double eps, double alpha, const double *sums,
                                 double n_den, float *dY, hipStream_t st) {
  const long long n = (long long)B * HW * F;
  if (n <= 0 || !(n_den >= (double)n)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(crnn_loss_grad_kernel, dim3(blocks_of(n)), dim3(256), 0, st, yhat, y, n, B, HW, F, eps, alpha, sums, n_den, dY);
  return hipGetLastError();
}

}  // namespace cm
