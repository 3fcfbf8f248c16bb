// DiT4D_V4 training kernels (reference: models/backbones/DiT4D_V4.py:106-204 in train mode, models/diffusion/ddpm.py:111-154).
// The host plan lives in cm_dit4d_train_host.inc.  Everything DiT4D_V4 shares with DiT2D -- the token GEMMs, the backward GEMMs,
// LayerNorm, GELU, the column sums, the spatial attention as ditt_attn_* over (sample, slot) groups -- is cm_dit.hip's and
// cm_dit_train.hip's; here is what the block structure adds:
//   ditt4_tattn_fwd / bwd   temporal cross-attention per (sample, patch): keys / values the T_p <= 8 slots of the patch (row
//                           stride N_s), queries the slots >= qs, probabilities dropped (site 3)
//   ditt4_gate_rows         the temporal gated residual, which reaches the future slots' rows only
// Determinism as in cm_dit_train.hip: one writer per element, fixed summation order (ascending slots; fixed wave butterflies),
// no atomics.
//
// Dropout site 3 (the stream of cm_dit_train.hip): counter (key slot >> 2, sample, step, 0x80000000 | 3 << 29 | block << 16 |
// head << 10 | query token index in the sample), word key slot & 3.
#include "cm_kernels.h"

#include <math.h>

namespace cm {

namespace {

constexpr int TP_MAX = 8;   // temporal slots held in registers

__device__ __forceinline__ float wave_sum(float v) {
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the wave's (sample, patch, head); false past the last wave
__device__ __forceinline__ bool tattn_wave(const DitTrTAttnArgs &a, long long &b, int &patch, int &h) {
  const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= (long long)a.B * a.Ns * a.heads) return false;
  h = (int)(w % a.heads);
  const long long bp = w / a.heads;
  patch = (int)(bp % a.Ns);
  b = bp / a.Ns;
  return true;
}

// mask values of one query's T_p key slots
__device__ __forceinline__ void tattn_masks(const DitTrTAttnArgs &a, long long b, int h, int row, float mk[TP_MAX]) {
  ditt_drop4(a.dr, a.dr.sample_base + b, DITT_SITE_TATTN, h, row, 0, mk);
  if (a.Tp > 4) ditt_drop4(a.dr, a.dr.sample_base + b, DITT_SITE_TATTN, h, row, 1, mk + 4);
  else mk[4] = mk[5] = mk[6] = mk[7] = 1.f;
}

// dit_attn_temporal_kernel (cm_dit.hip) in train mode: lane = head channel, scores by wave reduction, softmax over the T_p keys,
// lse = max + log(den) kept per (query, head), the probabilities that enter P v dropped (the denominator is not).
__global__ __launch_bounds__(256) void ditt4_tattn_fwd_kernel(const DitTrTAttnArgs a) {
  const int d = threadIdx.x & 63;
  long long b; int patch, h;
  if (!tattn_wave(a, b, patch, h)) return;
  const int tok = a.Tp * a.Ns, nq = a.Tp - a.qs, E3 = 3 * a.E;
  const float *base = a.qkv + (b * tok + patch) * E3 + h * 64 + d;
  float k[TP_MAX], v[TP_MAX];
#pragma unroll
  for (int j = 0; j < TP_MAX; ++j) {
    k[j] = j < a.Tp ? base[(long long)j * a.Ns * E3 + a.E] : 0.f;
    v[j] = j < a.Tp ? base[(long long)j * a.Ns * E3 + 2 * a.E] : 0.f;
  }
  for (int qi = 0; qi < nq; ++qi) {
    const int slot = a.qs + qi, row = slot * a.Ns + patch;
    const float q = base[(long long)slot * a.Ns * E3] * 0.125f;
    float s[TP_MAX], mk[TP_MAX], mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < TP_MAX; ++j) {
      s[j] = wave_sum(q * k[j]);
      if (j < a.Tp) mx = fmaxf(mx, s[j]);
    }
    tattn_masks(a, b, h, row, mk);
    float den = 0.f, o = 0.f;
#pragma unroll
    for (int j = 0; j < TP_MAX; ++j)
      if (j < a.Tp) {
        const float e = expf(s[j] - mx);
        den += e;
        o = fmaf(e * mk[j], v[j], o);
      }
    a.out[((b * nq + qi) * a.Ns + patch) * a.E + h * 64 + d] = o / den;
    if (d == 0) a.lse[((b * a.Ns + patch) * a.heads + h) * nq + qi] = mx + logf(den);
  }
}

// The backward of one (sample, patch, head) in registers.  Per query q (ascending), with A = M P / (1 - p):
//   P_k = exp(s_k - lse) / sum_j exp(s_j - lse)   from the SAVED lse (no fresh maximum), renormalised in registers
//   dA_k = <dO_q, V_k>,  delta = sum_k A_k dA_k,  dS_k = P_k (M_k dA_k / (1 - p) - delta)
//   dV_k += A_k dO_q,  dK_k += dS_k Q_q / 8,  dQ_q = sum_k dS_k K_k / 8
// A row of dS sums to delta (1 - sum P): that is what the renormalisation and a delta built from the SAME dA are for.
// exp(s - lse) alone carries the rounding of lse as a common factor 1 + e (1e-5 at `kshift`'s logits), which leaves -e delta in
// the row sum, and a delta from <dO, O> leaves the rounding of each dA_k there; dQ multiplies the row sum by the K bias (64 at
// `kshift`: 1.5e-4 and 4.9e-5 of the in-projection's gradient, against a bound of 1.5e-5).
// and then the rows of the [rows][3E] in-projection gradient: dQ of the query slots as they come, dK and dV of every slot, and the
// zeros of the Q third of the past slots, whose rows are no query.
__global__ __launch_bounds__(256) void ditt4_tattn_bwd_kernel(const DitTrTAttnArgs a) {
  const int d = threadIdx.x & 63;
  long long b; int patch, h;
  if (!tattn_wave(a, b, patch, h)) return;
  const int tok = a.Tp * a.Ns, nq = a.Tp - a.qs, E3 = 3 * a.E;
  const long long off = (b * tok + patch) * E3 + h * 64 + d;
  const float *base = a.qkv + off;
  float *gbase = a.dqkv + off;
  float k[TP_MAX], v[TP_MAX], dk[TP_MAX], dv[TP_MAX];
#pragma unroll
  for (int j = 0; j < TP_MAX; ++j) {
    k[j] = j < a.Tp ? base[(long long)j * a.Ns * E3 + a.E] : 0.f;
    v[j] = j < a.Tp ? base[(long long)j * a.Ns * E3 + 2 * a.E] : 0.f;
    dk[j] = 0.f;
    dv[j] = 0.f;
  }
  for (int qi = 0; qi < nq; ++qi) {
    const int slot = a.qs + qi, row = slot * a.Ns + patch;
    const float q = base[(long long)slot * a.Ns * E3] * 0.125f;
    const float dO = a.dout[((b * nq + qi) * a.Ns + patch) * a.E + h * 64 + d];
    const float lse = a.lse[((b * a.Ns + patch) * a.heads + h) * nq + qi];
    float pr[TP_MAX], da[TP_MAX], mk[TP_MAX];
    tattn_masks(a, b, h, row, mk);
    float psum = 0.f, delta = 0.f;
#pragma unroll
    for (int j = 0; j < TP_MAX; ++j) {
      const float s = wave_sum(q * k[j]);
      da[j] = wave_sum(dO * v[j]);
      pr[j] = j < a.Tp ? expf(s - lse) : 0.f;
      psum += pr[j];
    }
    const float inv = 1.0f / psum;
#pragma unroll
    for (int j = 0; j < TP_MAX; ++j) {
      pr[j] *= inv;
      delta = fmaf(pr[j] * mk[j], da[j], delta);
    }
    float dq = 0.f;
#pragma unroll
    for (int j = 0; j < TP_MAX; ++j) {
      const float ds = pr[j] * (mk[j] * da[j] - delta);
      dv[j] = fmaf(pr[j] * mk[j], dO, dv[j]);
      dk[j] = fmaf(ds, q, dk[j]);          // q carries the 1 / 8
      dq = fmaf(ds, k[j], dq);
    }
    gbase[(long long)slot * a.Ns * E3] = dq * 0.125f;
  }
#pragma unroll
  for (int j = 0; j < TP_MAX; ++j)
    if (j < a.Tp) {
      float *g = gbase + (long long)j * a.Ns * E3;
      if (j < a.qs) g[0] = 0.f;
      g[a.E] = dk[j];
      g[2 * a.E] = dv[j];
    }
}

__global__ __launch_bounds__(256) void ditt4_gate_rows_kernel(const float *__restrict__ Xin, float *__restrict__ Xout,
                                                              const float *__restrict__ Yc, float *__restrict__ Gc,
                                                              const float *__restrict__ dX, const float *__restrict__ mod, int ldmod,
                                                              int off_gate, int B, int tok, int row0, int D) {
  const int n4 = D >> 2, fr = tok - row0;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (Xin) {
    if (i >= (long long)B * tok * n4) return;
    const long long r = i / n4, b = r / tok;
    const int c4 = (int)(i % n4), s = (int)(r % tok);
    float4 x = *(const float4 *)(Xin + r * D + 4 * c4);
    if (s >= row0) {
      const float4 g = *(const float4 *)(mod + b * ldmod + off_gate + 4 * c4);
      const float4 y = *(const float4 *)(Yc + (b * fr + s - row0) * D + 4 * c4);
      x = make_float4(x.x + g.x * y.x, x.y + g.y * y.y, x.z + g.z * y.z, x.w + g.w * y.w);
    }
    *(float4 *)(Xout + r * D + 4 * c4) = x;
  } else {
    if (i >= (long long)B * fr * n4) return;
    const long long rc = i / n4, b = rc / fr;
    const int c4 = (int)(i % n4);
    const float4 g = *(const float4 *)(mod + b * ldmod + off_gate + 4 * c4);
    const float4 dx = *(const float4 *)(dX + (b * tok + row0 + rc % fr) * D + 4 * c4);
    *(float4 *)(Gc + rc * D + 4 * c4) = make_float4(g.x * dx.x, g.y * dx.y, g.z * dx.z, g.w * dx.w);
  }
}

bool tattn_ok(const DitTrTAttnArgs &a) {
  return a.B >= 1 && a.Tp >= 1 && a.Tp <= TP_MAX && a.qs >= 0 && a.qs < a.Tp && a.Ns >= 1 && a.Tp * a.Ns <= 1024 &&
         a.E == 64 * a.heads && a.heads <= 64 && a.dr.block >= 0 && a.dr.block < 8192 &&
         ((long long)a.B * a.Ns * a.heads + 3) / 4 <= 0x7fffffffLL;
}

}  // namespace

hipError_t launch_ditt4_tattn_fwd(const DitTrTAttnArgs &a, hipStream_t st) {
  if (!tattn_ok(a)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ditt4_tattn_fwd_kernel, dim3((unsigned)(((long long)a.B * a.Ns * a.heads + 3) / 4)), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_ditt4_tattn_bwd(const DitTrTAttnArgs &a, hipStream_t st) {
  if (!tattn_ok(a)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ditt4_tattn_bwd_kernel, dim3((unsigned)(((long long)a.B * a.Ns * a.heads + 3) / 4)), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_ditt4_gate_rows(const float *Xin, float *Xout, const float *Yc, float *Gc, const float *dX, const float *mod,
                                  int ldmod, int off_gate, int B, int tok, int row0, int D, hipStream_t st) {
  if (D % 4 || row0 < 0 || row0 >= tok || B < 1) return hipErrorInvalidValue;
  const long long n = (long long)B * (Xin ? tok : tok - row0) * (D / 4);
  hipLaunchKernelGGL(ditt4_gate_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, Xin, Xout, Yc, Gc, dX, mod, ldmod,
                     off_gate, B, tok, row0, D);
  return hipGetLastError();
}

}  // namespace cm
