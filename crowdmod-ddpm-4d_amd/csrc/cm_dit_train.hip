// DiT2D training kernels (reference: models/backbones/DiT2D.py in train mode, models/flow_matching/flow_matching.py:104-157).
// The host plan lives in cm_dit_train_host.inc; the train-mode forward reuses dit_gemm_kernel (cm_dit.hip) for every product.
//
// What is here: the train-mode attention (log-sum-exp kept, probabilities dropped), its two-pass backward, the backward
// GEMM (dX = dY W and dW = dY^T A, both on v_mfma_f32_32x32x2_f32: exact fp32 products, so the error budget is summation order),
// and the element-wise / reduction kernels between them (LayerNorm + modulate, GELU, gates, SiLU, gathers, column sums).
// ditt_gemm_f16_kernel is the backward GEMM's sibling on v_mfma_f32_32x32x16_f16 for the token Linears of a DiT4D_V4 step under
// autocast (cm_dit4d_train_set_autocast): f16 operands, the same fp32 partials and reduce; DiT2D never takes it.
// Determinism as in cm_dit.hip: one writer per element, fixed summation order, no atomics; sums over the B * S rows are either
// one thread's fixed-order chain (segsum, float64) or fixed k ranges written as partials and added in ascending order (GEMM).
//
// Dropout: a mask value is a pure function of (seed, optimizer step, global sample, block, site, head, row, column):
//   Philox4x32-10, key (seed lo, seed hi), counter (column >> 2, sample, step, 0x80000000 | site << 29 | block << 16 | head << 10 | row),
//   word (column & 3) -> u = unit_float(word); keep iff u >= p, value 1 / (1 - p) in fp32.
// site 0: attention probabilities (row = query, column = key); 1: after GELU (row = token, column = hidden unit, head 0);
// 2: after fc2 (row = token, column = channel, head 0); 3: the temporal attention of DiT4D_V4 (cm_dit4d_train.hip), whose spatial
// attention runs the kernels below per (sample, slot) group and draws at the group's place in its sample (DitDrop::gps).  Bit 31 of the fourth counter word keeps these draws apart from the
// Dropout3d masks (0xD120) and from philox_normal ((sample >> 32) ^ 0x5eed < 2^31).
#include "cm_kernels.h"
#include "cm_dit_f16.h"

#include <math.h>

#include <algorithm>

namespace cm {

typedef float ditt_f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int GB = 64, GK = 32, GS = GK + 1;

__device__ __forceinline__ double wave_sum_d(double v) {
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ int acc_row(int r, int hf) { return (r & 3) + 8 * (r >> 2) + 4 * hf; }

// ---- backward GEMM -------------------------------------------------------------------------------------------------
template <int TA>
__global__ __launch_bounds__(256) void ditt_gemm_kernel(const DitTrGemmArgs a) {
  __shared__ float As[GB * GS], Bs[GB * GS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long m0 = (long long)blockIdx.x * GB;
  const int n0 = blockIdx.y * GB, z = blockIdx.z;
  const long long kbeg = (long long)z * a.kchunk, kend = min(a.K, kbeg + a.kchunk);
  ditt_f32x16 acc;
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  const int wm = wave & 1, wn = wave >> 1;
  const int tk = tid >> 3, tg = (tid & 7) * 8;    // staging along the contiguous m / n direction: one k, eight columns
  const int sr = tid >> 2, sk = (tid & 3) * 8;    // staging along k: one row, eight k
  for (long long k0 = kbeg; k0 < kend; k0 += GK) {
    if (TA) {
      const long long k = k0 + tk;
      for (int e = 0; e < 8; ++e) {
        const long long m = m0 + tg + e;
        As[(tg + e) * GS + tk] = (k < kend && m < a.M) ? a.A[k * a.lda + m] : 0.f;
      }
    } else {
      const long long m = m0 + sr;
      for (int e = 0; e < 8; ++e) {
        const long long k = k0 + sk + e;
        As[sr * GS + sk + e] = (m < a.M && k < kend) ? a.A[m * a.lda + k] : 0.f;
      }
    }
    {
      const long long k = k0 + tk;
      for (int e = 0; e < 8; ++e) {
        const int n = n0 + tg + e;
        Bs[(tg + e) * GS + tk] = (k < kend && n < a.N) ? a.B[k * a.ldb + n] : 0.f;
      }
    }
    __syncthreads();
    const float *ap = As + (wm * 32 + (lane & 31)) * GS + (lane >> 5);
    const float *bp = Bs + (wn * 32 + (lane & 31)) * GS + (lane >> 5);
#pragma unroll
    for (int kk = 0; kk < GK; kk += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[kk], bp[kk], acc, 0, 0, 0);
    __syncthreads();
  }
  const int col = n0 + wn * 32 + (lane & 31);
  if (col >= a.N) return;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const long long rl = m0 + wm * 32 + acc_row(i, lane >> 5);
    if (rl >= a.M) continue;
    if (a.nsplit > 1) {
      a.part[((long long)z * a.M + rl) * a.N + col] = acc[i];
    } else {
      float *c = a.C + rl * a.ldc + col;
      *c = a.accum ? *c + acc[i] : acc[i];
    }
  }
}

// Two adjacent columns c, c + 1 of eight consecutive k rows of the row-major matrix P [k][ld]: x = column c, y = column c + 1,
// element j = row k + j; zeros at and past kend / cmax.
__device__ __forceinline__ void dh_load_t8(const float *__restrict__ P, int ld, long long k, long long kend, long long c, long long cmax,
                                           float x[8], float y[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    x[j] = y[j] = 0.f;
    if (k + j < kend && c < cmax) {
      const float *q = P + (k + j) * ld + c;
      if (c + 1 < cmax && (((uintptr_t)q) & 7) == 0) {
        const float2 t = *(const float2 *)q;
        x[j] = t.x; y[j] = t.y;
      } else {
        x[j] = q[0];
        if (c + 1 < cmax) y[j] = q[1];
      }
    }
  }
}

// The f16-operand sibling of ditt_gemm_kernel for the token Linears of an autocast training step (DitTrGemmArgs::f16): the same
// arguments, tile, k ranges and fp32 partials; dY, W and the saved A operand are rounded to f16 when staged (cm_dit_f16.h), and a
// k past the range's end is staged as zero (wgrad's K is a row count, a multiple of nothing).
// The instruction wants k contiguous per lane, but the contraction index is the slow index of W in dX = dY W and of both operands
// in dW = dY^T A.  Transposing staging: thread -> column pair 2 np, 2 np + 1 (np = tid & 31) and k group 8 (tid >> 5); it reads the
// pair as one 8-byte load from each of its eight k rows (a wave reads 256 contiguous bytes of two k rows per instruction), so it
// holds eight consecutive k of two columns and stores each as one 16-byte ds_write_b128 into the [column][k] image.  A store is
// served in groups of 8 consecutive lanes; lanes np & 4 store their odd column first and the others their even one, so the 8 rows
// of a group are 16 g + {0, 2, 4, 6, 9, 11, 13, 15} (then {1, 3, 5, 7, 8, 10, 12, 14}): distinct mod 8, conflict-free at 144-byte rows.
template <int TA>
__global__ __launch_bounds__(256) void ditt_gemm_f16_kernel(const DitTrGemmArgs a) {
  __shared__ __attribute__((aligned(16))) _Float16 As[GB * DH_S], Bs[GB * DH_S];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long m0 = (long long)blockIdx.x * GB;
  const int n0 = blockIdx.y * GB, z = blockIdx.z;
  const long long kbeg = (long long)z * a.kchunk, kend = min(a.K, kbeg + a.kchunk);
  ditt_f32x16 acc;
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  const int wm = wave & 1, wn = wave >> 1;
  const int np = tid & 31, tk = (tid >> 5) * 8, odd = (np >> 2) & 1;   // transposing staging
  const int sr = tid >> 3, sk = (tid & 7) * 8;                          // staging along k: rows sr and sr + 32, eight k
  // the chunk in flight: raw fp32 values in registers, fetched one chunk ahead so that the global loads run under the matrix
  // instructions of the chunk before; they are rounded when they are stored to LDS
  float ax[8], ay[8], bx[8], by[8];
  auto fetch = [&](long long k0) {
    if (TA) {
      dh_load_t8(a.A, a.lda, k0 + tk, kend, m0 + 2 * np, a.M, ax, ay);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) ax[e] = ay[e] = 0.f;
      if (m0 + sr < a.M) dh_load8(a.A + (m0 + sr) * a.lda, k0 + sk, kend, ax);
      if (m0 + sr + 32 < a.M) dh_load8(a.A + (m0 + sr + 32) * a.lda, k0 + sk, kend, ay);
    }
    dh_load_t8(a.B, a.ldb, k0 + tk, kend, n0 + 2 * np, a.N, bx, by);
  };
  fetch(kbeg);
  for (long long k0 = kbeg; k0 < kend; k0 += DH_K) {
    if (TA) {
      *(dit_f16x8 *)(As + (2 * np + odd) * DH_S + tk) = dh_round8(odd ? ay : ax);
      *(dit_f16x8 *)(As + (2 * np + 1 - odd) * DH_S + tk) = dh_round8(odd ? ax : ay);
    } else {
      *(dit_f16x8 *)(As + sr * DH_S + sk) = dh_round8(ax);
      *(dit_f16x8 *)(As + (sr + 32) * DH_S + sk) = dh_round8(ay);
    }
    *(dit_f16x8 *)(Bs + (2 * np + odd) * DH_S + tk) = dh_round8(odd ? by : bx);
    *(dit_f16x8 *)(Bs + (2 * np + 1 - odd) * DH_S + tk) = dh_round8(odd ? bx : by);
    __syncthreads();
    if (k0 + DH_K < kend) fetch(k0 + DH_K);
    acc = dh_mfma_chunk(As + (wm * 32 + (lane & 31)) * DH_S + 8 * (lane >> 5), Bs + (wn * 32 + (lane & 31)) * DH_S + 8 * (lane >> 5), acc);
    __syncthreads();
  }
  const int col = n0 + wn * 32 + (lane & 31);
  if (col >= a.N) return;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const long long rl = m0 + wm * 32 + acc_row(i, lane >> 5);
    if (rl >= a.M) continue;
    if (a.nsplit > 1) {
      a.part[((long long)z * a.M + rl) * a.N + col] = acc[i];
    } else {
      float *c = a.C + rl * a.ldc + col;
      *c = a.accum ? *c + acc[i] : acc[i];
    }
  }
}

__global__ __launch_bounds__(256) void ditt_gemm_reduce_kernel(const DitTrGemmArgs a) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x, mn = (long long)a.M * a.N;
  if (i >= mn) return;
  float *c = a.C + (i / a.N) * a.ldc + i % a.N;
  float s = a.accum ? *c : 0.f;
  for (int z = 0; z < a.nsplit; ++z) s += a.part[(long long)z * mn + i];
  *c = s;
}

// ---- segment column sums -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ditt_segsum_kernel(const float *__restrict__ U, int ldu, const float *__restrict__ V, int ldv,
                                                          float *__restrict__ out, int ldo, long long seg_rows, int N,
                                                          long long useg, long long vseg) {
  __shared__ double sh[8][32];
  const int tid = threadIdx.x, cl = tid & 31, j = tid >> 5;
  const int col = blockIdx.x * 32 + cl;
  const long long seg = blockIdx.y, u0 = seg * useg, v0 = seg * vseg;
  double s = 0.0;
  if (col < N)
    for (long long r = j; r < seg_rows; r += 8) {
      const double u = U[(u0 + r) * ldu + col];
      s += V ? u * (double)V[(v0 + r) * ldv + col] : u;
    }
  sh[j][cl] = s;
  __syncthreads();
  if (j == 0 && col < N) {
    double t = sh[0][cl];
    for (int k = 1; k < 8; ++k) t += sh[k][cl];
    out[seg * ldo + col] = (float)t;
  }
}

// Column sums over many rows in two stages: fixed row ranges as float64 partials [nseg][N], then their sum in ascending order.
__global__ __launch_bounds__(256) void ditt_colsum_part_kernel(const float *__restrict__ U, int ldu, double *__restrict__ part,
                                                               long long rows, long long seg_rows, int N) {
  __shared__ double sh[8][32];
  const int tid = threadIdx.x, cl = tid & 31, j = tid >> 5;
  const int col = blockIdx.x * 32 + cl;
  const long long r0 = (long long)blockIdx.y * seg_rows, r1 = min(rows, r0 + seg_rows);
  double s = 0.0;
  if (col < N)
    for (long long r = r0 + j; r < r1; r += 8) s += U[r * ldu + col];
  sh[j][cl] = s;
  __syncthreads();
  if (j == 0 && col < N) {
    double t = sh[0][cl];
    for (int k = 1; k < 8; ++k) t += sh[k][cl];
    part[(long long)blockIdx.y * N + col] = t;
  }
}

__global__ __launch_bounds__(256) void ditt_colsum_final_kernel(const double *__restrict__ part, float *__restrict__ out, int nseg, int N) {
  const int col = blockIdx.x * 256 + threadIdx.x;
  if (col >= N) return;
  double t = 0.0;
  for (int z = 0; z < nseg; ++z) t += part[(long long)z * N + col];
  out[col] = (float)t;
}

// ---- LayerNorm + modulate ------------------------------------------------------------------------------------------
__device__ __forceinline__ long long ln_phys(const DitTrLnArgs &a, long long r) {
  return (r / a.grp) * (long long)a.grp_stride + a.grp_off + r % a.grp;
}

__global__ __launch_bounds__(256) void ditt_ln_fwd_kernel(const DitTrLnArgs a) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= a.M) return;
  const long long pr = ln_phys(a, r);
  const float *x = a.X + pr * a.D;
  const float *mrow = a.mod + (pr / a.tok) * (long long)a.ldmod;
  double s = 0.0;
  for (int k = lane; k < a.D; k += 64) s += x[k];
  const double mu = wave_sum_d(s) / a.D;
  double q = 0.0;
  for (int k = lane; k < a.D; k += 64) { const double d = x[k] - mu; q += d * d; }
  const double rs = 1.0 / sqrt(wave_sum_d(q) / a.D + 1e-6);
  for (int k = lane; k < a.D; k += 64) {
    const float xn = (float)((x[k] - mu) * rs);
    a.XN[r * a.D + k] = xn;
    a.A[r * a.D + k] = xn * (1.0f + mrow[a.off_scale + k]) + mrow[a.off_shift + k];
  }
  if (lane == 0) a.rs[r] = (float)rs;
}

// dx = rstd (g - mean(g) - xn mean(g xn)), g = dA (1 + scale): the mean and variance terms of the normalisation
__global__ __launch_bounds__(256) void ditt_ln_bwd_kernel(const DitTrLnArgs a) {
  const int lane = threadIdx.x & 63;
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= a.M) return;
  const long long pr = ln_phys(a, r);
  const float *mrow = a.mod + (pr / a.tok) * (long long)a.ldmod + a.off_scale;
  const float *da = a.dA + r * a.D, *xn = a.XN + r * a.D;
  double s1 = 0.0, s2 = 0.0;
  for (int k = lane; k < a.D; k += 64) {
    const double g = (double)da[k] * (1.0 + (double)mrow[k]);
    s1 += g;
    s2 += g * xn[k];
  }
  const double m1 = wave_sum_d(s1) / a.D, m2 = wave_sum_d(s2) / a.D, rs = a.rs[r];
  float *dx = a.dX + pr * a.D;
  for (int k = lane; k < a.D; k += 64) {
    const double g = (double)da[k] * (1.0 + (double)mrow[k]);
    dx[k] += (float)(rs * (g - m1 - xn[k] * m2));
  }
}

// ---- element-wise --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ditt_gelu_drop_kernel(const float *__restrict__ H1, float *__restrict__ Hm, long long rows,
                                                             int N, int tok, DitDrop dr, int bwd) {
  const int n4 = N >> 2;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * n4) return;
  const long long r = i / n4;
  const int c4 = (int)(i % n4);
  float mk[4];
  ditt_drop4(dr, dr.sample_base + r / tok, DITT_SITE_MLP1, 0, (int)(r % tok), c4, mk);
  const float4 h = *(const float4 *)(H1 + r * N + 4 * c4);
  const float hv[4] = {h.x, h.y, h.z, h.w};
  float4 *dst = (float4 *)(Hm + r * N + 4 * c4);
  float dv[4] = {0.f, 0.f, 0.f, 0.f};
  if (bwd) { const float4 d = *dst; dv[0] = d.x; dv[1] = d.y; dv[2] = d.z; dv[3] = d.w; }
  float o[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float x = hv[e], cdf = 0.5f * (1.0f + erff(x * 0.70710678118654752f));
    if (bwd) o[e] = dv[e] * mk[e] * (cdf + x * expf(-0.5f * x * x) * 0.3989422804014327f);
    else o[e] = x * cdf * mk[e];
  }
  *dst = make_float4(o[0], o[1], o[2], o[3]);
}

__global__ __launch_bounds__(256) void ditt_gate_kernel(const float *__restrict__ Xin, float *__restrict__ Xout, float *__restrict__ Y,
                                                        const float *__restrict__ dX, const float *__restrict__ mod, int ldmod,
                                                        int off_gate, long long rows, int D, int tok, int site, DitDrop dr) {
  const int n4 = D >> 2;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * n4) return;
  const long long r = i / n4, b = r / tok;
  const int c4 = (int)(i % n4);
  float mk[4] = {1.f, 1.f, 1.f, 1.f};
  if (site != DITT_SITE_NONE) ditt_drop4(dr, dr.sample_base + b, site, 0, (int)(r % tok), c4, mk);
  const float4 g = *(const float4 *)(mod + b * ldmod + off_gate + 4 * c4);
  float4 *yp = (float4 *)(Y + r * D + 4 * c4);
  if (Xin) {
    float4 y = *yp;
    y.x *= mk[0]; y.y *= mk[1]; y.z *= mk[2]; y.w *= mk[3];
    if (site != DITT_SITE_NONE) *yp = y;
    const float4 x = *(const float4 *)(Xin + r * D + 4 * c4);
    *(float4 *)(Xout + r * D + 4 * c4) = make_float4(x.x + g.x * y.x, x.y + g.y * y.y, x.z + g.z * y.z, x.w + g.w * y.w);
  } else {
    const float4 d = *(const float4 *)(dX + r * D + 4 * c4);
    *yp = make_float4(g.x * d.x * mk[0], g.y * d.y * mk[1], g.z * d.z * mk[2], g.w * d.w * mk[3]);
  }
}

__global__ __launch_bounds__(256) void ditt_silu_kernel(const float *__restrict__ x, float *__restrict__ y, const float *__restrict__ dy,
                                                        long long n) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float v = x[i], sg = 1.0f / (1.0f + expf(-v));
  y[i] = dy ? dy[i] * (sg * (1.0f + v * (1.0f - sg))) : v * sg;
}

__global__ __launch_bounds__(256) void ditt_gather_rows_kernel(const float *__restrict__ table, const long long *__restrict__ t,
                                                               float *__restrict__ out, int B, int D) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)B * D) return;
  out[i] = table[t[i / D] * D + i % D];
}

// patches of the forward's gather prologue: k = ((c pt + it) p + ih) p + iw of token (slot, h_p, w_p), frame slot * pt + it
__global__ __launch_bounds__(256) void ditt_patch_gather_kernel(const DitTrPatchArgs a) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x, rows = (long long)a.B * a.tok;
  if (i >= rows * a.Kp) return;
  const long long pr = i / a.Kp, b = pr / a.tok;
  const int k = (int)(i % a.Kp), p = a.p;
  const int iw = k % p, ih = (k / p) % p, it = (k / (p * p)) % a.pt, c = k / (p * p * a.pt);
  const int s = (int)(pr % a.tok), tp = s / a.Ns, hw = s % a.Ns, hp = hw / a.wpn, wp = hw % a.wpn;
  a.Pm[i] = a.x8[((((b * a.L) + tp * a.pt + it) * a.Hh + hp * p + ih) * a.Ww + wp * p + iw) * 8 + c];
}

// d loss / d (final linear output) through the unpatchify gather: 2 (pred - target) / N at the voxel the feature lands on.
// Feature ((it C + c) p + ih) p + iw of future slot f is frame (qs + f) pt + it; a frame < P of the first future slot carries no
// loss: exactly 0.
__global__ __launch_bounds__(256) void ditt_loss_grad_kernel(const DitTrPatchArgs a) {
  const int nq = a.tok / a.Ns - a.qs, F = a.L - a.P, p = a.p;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x, rows = (long long)a.B * nq * a.Ns;
  if (i >= rows * a.Nout) return;
  const long long rc = i / a.Nout, b = rc / ((long long)nq * a.Ns);
  const int col = (int)(i % a.Nout), rem = (int)(rc % ((long long)nq * a.Ns)), sl = rem / a.Ns, hw = rem % a.Ns;
  const int iw = col % p, ih = (col / p) % p, c = (col / (p * p)) % a.C, it = col / (p * p * a.C);
  const int hp = hw / a.wpn, wp = hw % a.wpn, f = (a.qs + sl) * a.pt + it - a.P;
  if (f < 0) { a.dYf[i] = 0.f; return; }
  const long long e = ((((b * a.C + c) * a.Hh + hp * p + ih) * a.Ww + wp * p + iw) * F + f);
  const double n = (double)a.B * a.C * a.Hh * a.Ww * F;
  a.dYf[i] = (float)(((double)a.pred[e] - (double)a.target[e]) * ldexp(2.0 / n, a.ls_k));   // autocast: times the loss scale 2^ls_k
}

// spatial_pos_embed sums over batch and frames, temporal_pos_embed over batch and patches (rows >= T_p are left as they are: 0)
__global__ __launch_bounds__(256) void ditt_pos_grad_kernel(const DitTrPatchArgs a) {
  const int Tp = a.tok / a.Ns;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x, ns = (long long)a.Ns * a.D;
  if (i >= ns + (long long)Tp * a.D) return;
  double s = 0.0;
  if (i < ns) {
    const int hw = (int)(i / a.D), d = (int)(i % a.D);
    for (int b = 0; b < a.B; ++b)
      for (int tp = 0; tp < Tp; ++tp) s += a.dX0[((long long)b * a.tok + tp * a.Ns + hw) * a.D + d];
    a.dspos[i] = (float)s;
  } else {
    const int tp = (int)((i - ns) / a.D), d = (int)((i - ns) % a.D);
    for (int b = 0; b < a.B; ++b)
      for (int hw = 0; hw < a.Ns; ++hw) s += a.dX0[((long long)b * a.tok + tp * a.Ns + hw) * a.D + d];
    a.dtpos[i - ns] = (float)s;
  }
}

// ---- attention -----------------------------------------------------------------------------------------------------
// A row of q | k | v (or of a gradient with row stride ld) as the operand of the 32 steps of a 64-channel contraction: step s
// of half hf takes channel 2 s + hf.
__device__ __forceinline__ void load_op(const float *row, int hf, float scale, float out[32]) {
  const float4 *p = (const float4 *)row;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const float4 v = p[i];
    out[2 * i] = (hf ? v.y : v.x) * scale;
    out[2 * i + 1] = (hf ? v.w : v.z) * scale;
  }
}

// dit_attn_full_kernel (cm_dit.hip) in train mode: the same streaming softmax, plus lse = m + log(den) per query, and the
// probabilities that enter P v are dropped (the denominator is not: nn.MultiheadAttention drops softmax(s)).
__global__ __launch_bounds__(64) void ditt_attn_fwd_kernel(const DitTrAttnArgs a) {
  const int lane = threadIdx.x, c = lane & 31, hf = lane >> 5;
  const int S = a.S, nqt = (S + 31) / 32, E3 = 3 * a.E;
  const int qt = blockIdx.x % nqt;
  const long long bh = blockIdx.x / nqt;
  const int h = (int)(bh % a.heads);
  const long long b = bh / a.heads;
  const float *base = a.qkv + b * S * E3 + h * 64;
  const int q = qt * 32 + c, qc = min(q, S - 1);
  float qv[32], kc[32];
  load_op(base + (long long)qc * E3, hf, 0.125f, qv);
  float m = -INFINITY, den = 0.f;
  ditt_f32x16 o0, o1;
#pragma unroll
  for (int r = 0; r < 16; ++r) { o0[r] = 0.f; o1[r] = 0.f; }
  const float *vb = base + 2 * a.E + c;
  for (int k0 = 0; k0 < S; k0 += 32) {
    load_op(base + a.E + (long long)min(k0 + c, S - 1) * E3, hf, 1.f, kc);
    float v0[16], v1[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float *vr = vb + (long long)min(k0 + acc_row(r, hf), S - 1) * E3;
      v0[r] = vr[0];
      v1[r] = vr[32];
    }
    ditt_f32x16 s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
    for (int i = 0; i < 32; ++i) s = __builtin_amdgcn_mfma_f32_32x32x2f32(kc[i], qv[i], s, 0, 0, 0);
    float cmax = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      if (k0 + acc_row(r, hf) >= S) s[r] = -INFINITY;
      cmax = fmaxf(cmax, s[r]);
    }
    cmax = fmaxf(cmax, __shfl_xor(cmax, 32, 64));
    const float mn = fmaxf(m, cmax);
    const float alpha = expf(m - mn);
    float csum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) { s[r] = expf(s[r] - mn); csum += s[r]; }
    csum += __shfl_xor(csum, 32, 64);
    den = den * alpha + csum;
    m = mn;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float mk[4];
      ditt_drop4(a.dr, a.dr.sample_base + b / a.dr.gps, DITT_SITE_ATTN, h, (int)(b % a.dr.gps) * S + qc, (k0 + 8 * g + 4 * hf) >> 2, mk);
#pragma unroll
      for (int e = 0; e < 4; ++e) s[4 * g + e] *= mk[e];
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) { o0[r] *= alpha; o1[r] *= alpha; }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(v0[r], s[r], o0, 0, 0, 0);
      o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(v1[r], s[r], o1, 0, 0, 0);
    }
  }
  if (q >= S) return;
  if (hf == 0) a.lse[(b * a.heads + h) * S + q] = m + logf(den);
  float *orow = a.out + (b * S + q) * a.E + h * 64 + 4 * hf;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    *(float4 *)(orow + 8 * g) = make_float4(o0[4 * g] / den, o0[4 * g + 1] / den, o0[4 * g + 2] / den, o0[4 * g + 3] / den);
    *(float4 *)(orow + 32 + 8 * g) = make_float4(o1[4 * g] / den, o1[4 * g + 1] / den, o1[4 * g + 2] / den, o1[4 * g + 3] / den);
  }
}

// delta[b][h][q] = sum_d dO[q][d] O[q][d] (= sum_k P dP also under dropout, because O = A V): one wave per (token row, head)
__global__ __launch_bounds__(256) void ditt_attn_delta_kernel(const DitTrAttnArgs a) {
  const int lane = threadIdx.x & 63;
  const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6), nw = (long long)a.B * a.S * a.heads;
  if (w >= nw) return;
  const int h = (int)(w % a.heads);
  const long long row = w / a.heads, b = row / a.S;
  const long long i = row * a.E + h * 64 + lane;
  const double s = wave_sum_d((double)a.dout[i] * (double)a.out[i]);
  if (lane == 0) a.delta[(b * a.heads + h) * a.S + row % a.S] = (float)s;
}

// dQ: one wave per (sample, head, 32-query tile), key chunks streamed.  Per chunk
//   S^T  = k q^T / 8, dA^T = v dO^T    (a lane's 16 values: 16 keys of its query, as in the forward)
//   P^T  = exp(S^T - lse), dS^T = P^T (M dA^T / (1 - p) - delta)
//   dQ^T += k^T dS^T                   (dS^T goes from the accumulator registers into the B operand, like P in the forward)
__global__ __launch_bounds__(64) void ditt_attn_dq_kernel(const DitTrAttnArgs a) {
  const int lane = threadIdx.x, c = lane & 31, hf = lane >> 5;
  const int S = a.S, nqt = (S + 31) / 32, E3 = 3 * a.E;
  const int qt = blockIdx.x % nqt;
  const long long bh = blockIdx.x / nqt;
  const int h = (int)(bh % a.heads);
  const long long b = bh / a.heads;
  const float *base = a.qkv + b * S * E3 + h * 64;
  const int q = qt * 32 + c, qc = min(q, S - 1);
  float qv[32], dov[32], kc[32], vc[32];
  load_op(base + (long long)qc * E3, hf, 0.125f, qv);
  load_op(a.dout + (b * S + qc) * a.E + h * 64, hf, 1.f, dov);
  const float lse = a.lse[(b * a.heads + h) * S + qc], dl = a.delta[(b * a.heads + h) * S + qc];
  ditt_f32x16 g0, g1;
#pragma unroll
  for (int r = 0; r < 16; ++r) { g0[r] = 0.f; g1[r] = 0.f; }
  const float *kb = base + a.E + c;
  for (int k0 = 0; k0 < S; k0 += 32) {
    const long long krow = (long long)min(k0 + c, S - 1) * E3;
    load_op(base + a.E + krow, hf, 1.f, kc);
    load_op(base + 2 * a.E + krow, hf, 1.f, vc);
    float t0[16], t1[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float *kr = kb + (long long)min(k0 + acc_row(r, hf), S - 1) * E3;
      t0[r] = kr[0];
      t1[r] = kr[32];
    }
    ditt_f32x16 s, da;
#pragma unroll
    for (int r = 0; r < 16; ++r) { s[r] = 0.f; da[r] = 0.f; }
#pragma unroll
    for (int i = 0; i < 32; ++i) {
      s = __builtin_amdgcn_mfma_f32_32x32x2f32(kc[i], qv[i], s, 0, 0, 0);
      da = __builtin_amdgcn_mfma_f32_32x32x2f32(vc[i], dov[i], da, 0, 0, 0);
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float mk[4];
      ditt_drop4(a.dr, a.dr.sample_base + b / a.dr.gps, DITT_SITE_ATTN, h, (int)(b % a.dr.gps) * S + qc, (k0 + 8 * g + 4 * hf) >> 2, mk);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int r = 4 * g + e;
        const float p = k0 + acc_row(r, hf) < S ? expf(s[r] - lse) : 0.f;   // tail keys: weight exactly 0
        s[r] = p * (da[r] * mk[e] - dl);
      }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      g0 = __builtin_amdgcn_mfma_f32_32x32x2f32(t0[r], s[r], g0, 0, 0, 0);
      g1 = __builtin_amdgcn_mfma_f32_32x32x2f32(t1[r], s[r], g1, 0, 0, 0);
    }
  }
  if (q >= S) return;
  float *orow = a.dqkv + (b * S + q) * E3 + h * 64 + 4 * hf;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    *(float4 *)(orow + 8 * g) = make_float4(g0[4 * g] * 0.125f, g0[4 * g + 1] * 0.125f, g0[4 * g + 2] * 0.125f, g0[4 * g + 3] * 0.125f);
    *(float4 *)(orow + 32 + 8 * g) = make_float4(g1[4 * g] * 0.125f, g1[4 * g + 1] * 0.125f, g1[4 * g + 2] * 0.125f, g1[4 * g + 3] * 0.125f);
  }
}

// dK, dV: one wave per (sample, head, 32-key tile), query chunks streamed.  Per chunk
//   S  = q k^T / 8, dA = dO v^T        (a lane's 16 values: 16 queries of its key)
//   A  = M P / (1 - p), dS = P (M dA / (1 - p) - delta)
//   dV^T += dO^T A, dK^T += q^T dS     (A and dS from the accumulator registers)
__global__ __launch_bounds__(64) void ditt_attn_dkv_kernel(const DitTrAttnArgs a) {
  const int lane = threadIdx.x, c = lane & 31, hf = lane >> 5;
  const int S = a.S, nkt = (S + 31) / 32, E3 = 3 * a.E;
  const int kt = blockIdx.x % nkt;
  const long long bh = blockIdx.x / nkt;
  const int h = (int)(bh % a.heads);
  const long long b = bh / a.heads;
  const float *base = a.qkv + b * S * E3 + h * 64;
  const float *dob = a.dout + b * S * a.E + h * 64;
  const float *lseb = a.lse + (b * a.heads + h) * S, *dlb = a.delta + (b * a.heads + h) * S;
  const int key = kt * 32 + c, kcl = min(key, S - 1);
  float kv[32], vv[32], qa[32], da_op[32];
  load_op(base + a.E + (long long)kcl * E3, hf, 0.125f, kv);
  load_op(base + 2 * a.E + (long long)kcl * E3, hf, 1.f, vv);
  ditt_f32x16 gk0, gk1, gv0, gv1;
#pragma unroll
  for (int r = 0; r < 16; ++r) { gk0[r] = 0.f; gk1[r] = 0.f; gv0[r] = 0.f; gv1[r] = 0.f; }
  for (int q0 = 0; q0 < S; q0 += 32) {
    const int qrow = min(q0 + c, S - 1);
    load_op(base + (long long)qrow * E3, hf, 1.f, qa);
    load_op(dob + (long long)qrow * a.E, hf, 1.f, da_op);
    ditt_f32x16 s, da;
#pragma unroll
    for (int r = 0; r < 16; ++r) { s[r] = 0.f; da[r] = 0.f; }
#pragma unroll
    for (int i = 0; i < 32; ++i) {
      s = __builtin_amdgcn_mfma_f32_32x32x2f32(qa[i], kv[i], s, 0, 0, 0);
      da = __builtin_amdgcn_mfma_f32_32x32x2f32(da_op[i], vv[i], da, 0, 0, 0);
    }
    float t0[16], t1[16], u0[16], u1[16];
    ditt_f32x16 pa;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int qr = q0 + acc_row(r, hf), qrc = min(qr, S - 1);
      const float *qp = base + (long long)qrc * E3 + c, *dp = dob + (long long)qrc * a.E + c;
      t0[r] = qp[0]; t1[r] = qp[32];
      u0[r] = dp[0]; u1[r] = dp[32];
      float mk[4];
      ditt_drop4(a.dr, a.dr.sample_base + b / a.dr.gps, DITT_SITE_ATTN, h, (int)(b % a.dr.gps) * S + qrc, key >> 2, mk);
      const float mv = mk[key & 3];
      const float p = qr < S ? expf(s[r] - lseb[qrc]) : 0.f;   // tail queries contribute exactly 0
      pa[r] = p * mv;
      s[r] = p * (da[r] * mv - dlb[qrc]);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      gv0 = __builtin_amdgcn_mfma_f32_32x32x2f32(u0[r], pa[r], gv0, 0, 0, 0);
      gv1 = __builtin_amdgcn_mfma_f32_32x32x2f32(u1[r], pa[r], gv1, 0, 0, 0);
      gk0 = __builtin_amdgcn_mfma_f32_32x32x2f32(t0[r], s[r], gk0, 0, 0, 0);
      gk1 = __builtin_amdgcn_mfma_f32_32x32x2f32(t1[r], s[r], gk1, 0, 0, 0);
    }
  }
  if (key >= S) return;
  float *krow = a.dqkv + (b * S + key) * E3 + a.E + h * 64 + 4 * hf;
  float *vrow = krow + a.E;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    *(float4 *)(krow + 8 * g) = make_float4(gk0[4 * g] * 0.125f, gk0[4 * g + 1] * 0.125f, gk0[4 * g + 2] * 0.125f, gk0[4 * g + 3] * 0.125f);
    *(float4 *)(krow + 32 + 8 * g) = make_float4(gk1[4 * g] * 0.125f, gk1[4 * g + 1] * 0.125f, gk1[4 * g + 2] * 0.125f, gk1[4 * g + 3] * 0.125f);
    *(float4 *)(vrow + 8 * g) = make_float4(gv0[4 * g], gv0[4 * g + 1], gv0[4 * g + 2], gv0[4 * g + 3]);
    *(float4 *)(vrow + 32 + 8 * g) = make_float4(gv1[4 * g], gv1[4 * g + 1], gv1[4 * g + 2], gv1[4 * g + 3]);
  }
}

unsigned blocks_of(long long n) { return (unsigned)((n + 255) / 256); }

}  // namespace

hipError_t launch_ditt_gemm(const DitTrGemmArgs &a, hipStream_t st) {
  if (a.M <= 0 || a.N <= 0) return hipSuccess;
  if (a.nsplit > 1 && (!a.part || a.kchunk % GK)) return hipErrorInvalidValue;
  DitTrGemmArgs k = a;
  if (k.nsplit <= 1) { k.nsplit = 1; k.kchunk = ((a.K + GK - 1) / GK) * GK; if (k.kchunk < GK) k.kchunk = GK; }
  dim3 grid((unsigned)((a.M + GB - 1) / GB), (unsigned)((a.N + GB - 1) / GB), (unsigned)k.nsplit);
  if (a.f16 && a.ta) hipLaunchKernelGGL((ditt_gemm_f16_kernel<1>), grid, dim3(256), 0, st, k);
  else if (a.f16) hipLaunchKernelGGL((ditt_gemm_f16_kernel<0>), grid, dim3(256), 0, st, k);
  else if (a.ta) hipLaunchKernelGGL((ditt_gemm_kernel<1>), grid, dim3(256), 0, st, k);
  else hipLaunchKernelGGL((ditt_gemm_kernel<0>), grid, dim3(256), 0, st, k);
  if (k.nsplit > 1) hipLaunchKernelGGL(ditt_gemm_reduce_kernel, dim3(blocks_of((long long)a.M * a.N)), dim3(256), 0, st, k);
  return hipGetLastError();
}

hipError_t launch_ditt_segsum(const float *U, int ldu, const float *V, int ldv, float *out, int ldo, int nseg, long long seg_rows,
                              int N, hipStream_t st) {
  if (nseg <= 0 || N <= 0) return hipSuccess;
  return launch_ditt_segsum_rows(U, ldu, seg_rows, V, ldv, seg_rows, out, ldo, nseg, seg_rows, N, st);
}

hipError_t launch_ditt_segsum_rows(const float *U, int ldu, long long useg, const float *V, int ldv, long long vseg, float *out,
                                   int ldo, int nseg, long long seg_rows, int N, hipStream_t st) {
  if (nseg <= 0 || N <= 0) return hipSuccess;
  hipLaunchKernelGGL(ditt_segsum_kernel, dim3((unsigned)((N + 31) / 32), (unsigned)nseg), dim3(256), 0, st, U, ldu, V, ldv, out, ldo,
                     seg_rows, N, useg, vseg);
  return hipGetLastError();
}

hipError_t launch_ditt_colsum(const float *U, int ldu, float *out, long long rows, int N, double *part, hipStream_t st) {
  if (N <= 0) return hipSuccess;
  if (rows <= DITT_COLSUM_ROWS) return launch_ditt_segsum(U, ldu, nullptr, 0, out, N, 1, rows, N, st);
  const int nseg = (int)std::min<long long>(DITT_COLSUM_SEGS, (rows + 63) / 64);
  const long long seg_rows = (rows + nseg - 1) / nseg;
  hipLaunchKernelGGL(ditt_colsum_part_kernel, dim3((unsigned)((N + 31) / 32), (unsigned)nseg), dim3(256), 0, st, U, ldu, part, rows,
                     seg_rows, N);
  hipLaunchKernelGGL(ditt_colsum_final_kernel, dim3(blocks_of(N)), dim3(256), 0, st, part, out, nseg, N);
  return hipGetLastError();
}

hipError_t launch_ditt_ln_fwd(const DitTrLnArgs &a, hipStream_t st) {
  if (a.M <= 0) return hipSuccess;
  hipLaunchKernelGGL(ditt_ln_fwd_kernel, dim3((unsigned)((a.M + 3) / 4)), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_ditt_ln_bwd(const DitTrLnArgs &a, hipStream_t st) {
  if (a.M <= 0) return hipSuccess;
  hipLaunchKernelGGL(ditt_ln_bwd_kernel, dim3((unsigned)((a.M + 3) / 4)), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_ditt_gelu_drop(const float *H1, float *Hm, long long rows, int N, int tok, DitDrop dr, int bwd, hipStream_t st) {
  if (N % 4) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ditt_gelu_drop_kernel, dim3(blocks_of(rows * (N / 4))), dim3(256), 0, st, H1, Hm, rows, N, tok, dr, bwd);
  return hipGetLastError();
}

hipError_t launch_ditt_gate(const float *Xin, float *Xout, float *Y, const float *dX, const float *mod, int ldmod, int off_gate,
                            long long rows, int D, int tok, int site, DitDrop dr, hipStream_t st) {
  if (D % 4) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ditt_gate_kernel, dim3(blocks_of(rows * (D / 4))), dim3(256), 0, st, Xin, Xout, Y, dX, mod, ldmod, off_gate, rows,
                     D, tok, site, dr);
  return hipGetLastError();
}

hipError_t launch_ditt_silu(const float *x, float *y, const float *dy, long long n, hipStream_t st) {
  hipLaunchKernelGGL(ditt_silu_kernel, dim3(blocks_of(n)), dim3(256), 0, st, x, y, dy, n);
  return hipGetLastError();
}

hipError_t launch_ditt_gather_rows(const float *table, const long long *t, float *out, int B, int D, hipStream_t st) {
  hipLaunchKernelGGL(ditt_gather_rows_kernel, dim3(blocks_of((long long)B * D)), dim3(256), 0, st, table, t, out, B, D);
  return hipGetLastError();
}

hipError_t launch_ditt_patch_gather(const DitTrPatchArgs &a, hipStream_t st) {
  if (a.pt < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ditt_patch_gather_kernel, dim3(blocks_of((long long)a.B * a.tok * a.Kp)), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_ditt_loss_grad(const DitTrPatchArgs &a, hipStream_t st) {
  if (a.pt < 1 || a.P < 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ditt_loss_grad_kernel, dim3(blocks_of((long long)a.B * (a.tok / a.Ns - a.qs) * a.Ns * a.Nout)), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_ditt_pos_grad(const DitTrPatchArgs &a, hipStream_t st) {
  hipLaunchKernelGGL(ditt_pos_grad_kernel, dim3(blocks_of((long long)(a.Ns + a.tok / a.Ns) * a.D)), dim3(256), 0, st, a);
  return hipGetLastError();
}

namespace {
bool attn_ok(const DitTrAttnArgs &a) {
  return a.S >= 1 && a.dr.gps >= 1 && (long long)a.dr.gps * a.S <= 1024 && a.E == 64 * a.heads && a.heads <= 64 && a.dr.block >= 0 && a.dr.block < 8192 &&
         (long long)a.B * a.heads * ((a.S + 31) / 32) <= 0x7fffffffLL;
}
}  // namespace

hipError_t launch_ditt_attn_fwd(const DitTrAttnArgs &a, hipStream_t st) {
  if (!attn_ok(a)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ditt_attn_fwd_kernel, dim3((unsigned)((long long)a.B * a.heads * ((a.S + 31) / 32))), dim3(64), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_ditt_attn_delta(const DitTrAttnArgs &a, hipStream_t st) {
  if (!attn_ok(a)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ditt_attn_delta_kernel, dim3((unsigned)(((long long)a.B * a.S * a.heads + 3) / 4)), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_ditt_attn_bwd(const DitTrAttnArgs &a, hipStream_t st) {
  if (!attn_ok(a)) return hipErrorInvalidValue;
  const unsigned n = (unsigned)((long long)a.B * a.heads * ((a.S + 31) / 32));
  hipLaunchKernelGGL(ditt_attn_dq_kernel, dim3(n), dim3(64), 0, st, a);
  hipLaunchKernelGGL(ditt_attn_dkv_kernel, dim3(n), dim3(64), 0, st, a);
  return hipGetLastError();
}

}  // namespace cm
