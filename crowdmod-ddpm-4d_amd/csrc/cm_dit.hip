// DiT4D_V4 denoiser kernels (reference: models/backbones/DiT4D_V4.py).  The host plan lives in cm_dit_host.inc.
//
// Activations are token-major fp32 [B][T_p * N_s][D] (token order (t_p, h_p, w_p), DiT4D_V4.py:57-60); the residual
// stream is updated in place by the gated epilogues.  Two kinds of kernel carry the whole forward:
//   dit_gemm_kernel   Y = epilogue(prologue(A) W^T + b) on exact-fp32 matrix instructions (v_mfma_f32_32x32x2_f32),
//                     W in the reference [out][in] layout.  Prologues: plain rows, LayerNorm (no affine, eps 1e-6,
//                     biased variance) + modulate with the sample's row of the conditioning table, or the Conv3d
//                     patch gather from the channels-last sampler tensor x8.  Epilogues: bias, SiLU, SiLU(SiLU(.))
//                     (conditioning tables), exact-erf GELU, gated residual, patch embedding + both position
//                     embeddings, and the unpatchify scatter of the final linear into eps_cl.  A row subset (the
//                     temporal queries, the future slots of the final layer) maps logical GEMM rows to token rows.
//   dit_gemm_f16_kernel  its sibling on v_mfma_f32_32x32x16_f16 for the blocks' token Linears: operands rounded to f16, fp32
//                     accumulation and output.  Taken by the autocast TRAINING step (cm_dit4d_train_set_autocast; fp32 master
//                     weights rounded when staged) and by the eval forward of a handle on the f16 sampling plan
//                     (cm_model_set_precision(CM_PRECISION_F16); weights rounded once by dit_finalize); the default plan never takes it.
//   dit_attn_*        softmax(q k^T / 8) v per head (head dim 64) on the vector ALUs: spatial self-attention over the
//                     N_s tokens of one (sample, slot), temporal cross-attention of the future slots of one (sample,
//                     patch) over all T_p slots.
//   dit_attn_full     the DiT2D variant (models/backbones/DiT2D.py): one self-attention over all S = T_p * N_s tokens of
//                     a sample, q k^T and P v both on v_mfma_f32_32x32x2_f32 with a streaming softmax.
//   dit_attn_full_f16 the same attention with both products on v_mfma_f32_32x32x16_f16 (operands rounded to f16, fp32 softmax,
//                     denominator and accumulation): taken only by an FM-DiT handle on the f16a plan
//                     (cm_model_set_precision(CM_PRECISION_F16A)), whose four token Linears per block take dit_gemm_f16_kernel.
// Determinism: every output element is written by one thread with a fixed summation order (k ascending in one fma
// chain; fixed butterfly reductions), no atomics, and a sample only reads its own rows -- a chain's result does not
// depend on the batch it runs in, the batch lane, or graph replay.
#include "cm_kernels.h"
#include "cm_dit_f16.h"

#include <math.h>

namespace cm {

typedef float dit_f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int GB = 64;    // rows and columns of a workgroup tile (2 x 2 waves of 32 x 32)
constexpr int GK = 32;    // k chunk staged in LDS
constexpr int GS = GK + 1;
constexpr int TP_MAX = 8; // temporal slots the temporal-attention kernel holds in registers

__device__ __forceinline__ float wave_sum(float v) {
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ long long phys_row(const DitGemmArgs &a, long long r) {
  return (r / a.grp) * (long long)a.grp_stride + a.grp_off + r % a.grp;
}

__device__ __forceinline__ float silu(float x) { return x / (1.0f + expf(-x)); }

// LayerNorm statistics of the 64 token rows of the tile at m0 (K = D, the whole row), and each row's conditioning row: wave w
// owns rows 16w .. 16w + 15.  Shared by dit_gemm_kernel and dit_gemm_f16_kernel, so both normalise with the same bits.
__device__ __forceinline__ void ln_tile_stats(const DitGemmArgs &a, long long m0, int lane, int wave, float *s_mu, float *s_rs,
                                              const float **s_mod) {
  // Eight rows at a time, so that eight independent loads are in flight per k step instead of one: each row's sums keep their
  // order (k ascending per lane, then the butterfly), so the statistics are the bits of the one-row-at-a-time loop.  A row past M
  // reads row M - 1 and is discarded.
  constexpr int R = 8;
  for (int r0 = wave * 16; r0 < wave * 16 + 16; r0 += R) {
    const float *x[R];
    long long pr[R];
    float s[R], q[R], mu[R];
#pragma unroll
    for (int j = 0; j < R; ++j) {
      pr[j] = phys_row(a, min(m0 + r0 + j, a.M - 1));
      x[j] = a.A + pr[j] * a.lda;
      s[j] = q[j] = 0.f;
    }
    for (int k = lane; k < a.K; k += 64) {
#pragma unroll
      for (int j = 0; j < R; ++j) s[j] += x[j][k];
    }
#pragma unroll
    for (int j = 0; j < R; ++j) mu[j] = wave_sum(s[j]) / (float)a.K;
    for (int k = lane; k < a.K; k += 64) {
#pragma unroll
      for (int j = 0; j < R; ++j) { const float d = x[j][k] - mu[j]; q[j] += d * d; }
    }
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const bool ok = m0 + r0 + j < a.M;
      const float rs = 1.0f / sqrtf(wave_sum(q[j]) / (float)a.K + 1e-6f);
      if (lane == 0) {
        s_mu[r0 + j] = ok ? mu[j] : 0.f;
        s_rs[r0 + j] = ok ? rs : 0.f;
        s_mod[r0 + j] = ok ? a.mod + a.tbuf[pr[j] / a.tok] * (long long)a.ldmod : nullptr;
      }
    }
  }
}

template <int PRO, int EPI>
__global__ __launch_bounds__(256) void dit_gemm_kernel(const DitGemmArgs a) {
  __shared__ float As[GB * GS], Ws[GB * GS];
  __shared__ float s_mu[GB], s_rs[GB];
  __shared__ const float *s_mod[GB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long m0 = (long long)blockIdx.x * GB;
  const int n0 = blockIdx.y * GB;

  if (PRO == DIT_PRO_LN) {
    ln_tile_stats(a, m0, lane, wave, s_mu, s_rs, s_mod);
    __syncthreads();
  }

  dit_f32x16 acc;
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  const int wm = wave & 1, wn = wave >> 1;
  const int sr = tid >> 2, sk = (tid & 3) * 8;   // staging: one row, eight consecutive k per thread
  const long long r = m0 + sr;
  const bool rok = r < a.M;
  const long long pr = rok ? phys_row(a, r) : 0;
  const long long ar = a.a_compact ? r : pr;
  const int n = n0 + sr;
  for (int k0 = 0; k0 < a.K; k0 += GK) {
    for (int e = 0; e < 8; ++e) {
      const int k = k0 + sk + e;
      float v = 0.f;
      if (rok && k < a.K) {
        if (PRO == DIT_PRO_PATCH) {
          // Conv3d weight [D][C][pt][p][p] on x.permute(0,1,4,2,3) (DiT4D_V4.py:56-57): k = ((c*pt + it)*p + ih)*p + iw
          const int p = a.p, pt = a.pt;
          const int iw = k % p, ih = (k / p) % p, it = (k / (p * p)) % pt, c = k / (p * p * pt);
          const long long b = pr / a.tok;
          const int s = (int)(pr % a.tok), tp = s / a.Ns, hw = s % a.Ns;
          const int hp = hw / a.wpn, wp = hw % a.wpn;
          const int fr = tp * pt + it, y = hp * p + ih, x = wp * p + iw;
          v = a.x8[((((b * a.L) + fr) * a.Hh + y) * a.Ww + x) * 8 + c];
        } else if (PRO == DIT_PRO_LN) {
          const float *mrow = s_mod[sr];
          const float xn = (a.A[ar * a.lda + k] - s_mu[sr]) * s_rs[sr];
          v = xn * (1.0f + mrow[a.off_scale + k]) + mrow[a.off_shift + k];   // modulate, DiT4D_V4.py:101-103
        } else {
          v = a.A[ar * a.lda + k];
        }
      }
      As[sr * GS + sk + e] = v;
      Ws[sr * GS + sk + e] = (n < a.N && k < a.K) ? a.W[(long long)n * a.K + k] : 0.f;
    }
    __syncthreads();
    const float *ap = As + (wm * 32 + (lane & 31)) * GS + (lane >> 5);
    const float *bp = Ws + (wn * 32 + (lane & 31)) * GS + (lane >> 5);
#pragma unroll
    for (int kk = 0; kk < GK; kk += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[kk], bp[kk], acc, 0, 0, 0);
    __syncthreads();
  }

  // C/D map: column = lane & 31, row = (i & 3) + 8 (i >> 2) + 4 (lane >> 5)
  const int col = n0 + wn * 32 + (lane & 31);
  if (col >= a.N) return;
  const float bias = a.bias ? a.bias[col] : 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const long long rl = m0 + wm * 32 + (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
    if (rl >= a.M) continue;
    const long long prow = phys_row(a, rl);
    const float v = acc[i] + bias;
    if (EPI == DIT_EPI_BIAS) {
      a.Y[prow * a.ldy + col] = v;
    } else if (EPI == DIT_EPI_SILU) {
      a.Y[prow * a.ldy + col] = silu(v);
    } else if (EPI == DIT_EPI_SILU2) {
      a.Y[prow * a.ldy + col] = silu(silu(v));
    } else if (EPI == DIT_EPI_GELU) {
      a.Y[prow * a.ldy + col] = 0.5f * v * (1.0f + erff(v * 0.70710678118654752f));
    } else if (EPI == DIT_EPI_GATE) {
      const float *mrow = a.mod + a.tbuf[prow / a.tok] * (long long)a.ldmod;
      float *y = a.Y + prow * a.ldy + col;
      *y = *y + mrow[a.off_gate + col] * v;
    } else if (EPI == DIT_EPI_PATCH) {
      const int s = (int)(prow % a.tok), tp = s / a.Ns, hw = s % a.Ns;
      a.Y[prow * a.ldy + col] = v + a.spos[hw * a.N + col] + a.tpos[tp * a.N + col];
    } else {   // DIT_EPI_UNPATCH: feature ((it*C + c)*p + ih)*p + iw -> frame tp*pt + it, row hp*p + ih, col wp*p + iw
      const int p = a.p, pt = a.pt;
      const int iw = col % p, ih = (col / p) % p, c = (col / (p * p)) % a.Cout, it = col / (p * p * a.Cout);
      const long long b = prow / a.tok;
      const int s = (int)(prow % a.tok), tp = s / a.Ns, hw = s % a.Ns;
      const int hp = hw / a.wpn, wp = hw % a.wpn;
      const int fr = tp * pt + it, y = hp * p + ih, x = wp * p + iw;
      a.Y[((((b * a.L) + fr) * a.Hh + y) * a.Ww + x) * 8 + c] = v;
    }
  }
}

// The f16-operand sibling of dit_gemm_kernel for the blocks' token Linears (DitGemmArgs::f16): the same 64 x 64 tile, row-subset
// addressing and LayerNorm statistics; the A operand is the fp32 value dit_gemm_kernel would stage (LayerNorm + modulate in fp32,
// where torch's autocast casts it), rounded to f16 when staged.  Two weight sources:
//   WH = false  the autocast training step: the fp32 master weight a.W, rounded when staged like A; bias epilogue only
//   WH = true   the f16 sampling plan (cm_model_set_precision): a.Wh, the copy dit_finalize rounded once, [N][K] halves; one
//               16-byte load gives eight k of a row with no conversion (launch_dit_gemm admits K % 8 == 0 only, so a group is whole
//               and aligned).  Epilogues bias, GELU and gated residual, with dit_gemm_kernel's expressions.
// Layout, rounding and the bank arithmetic: cm_dit_f16.h.  Staging: thread -> row tid >> 3 (and + 32), k group 8 (tid & 7).
// Edges as dit_gemm_kernel: rows >= M, columns >= N and k >= K are staged as zeros.
template <int PRO, int EPI, bool WH>
__global__ __launch_bounds__(256) void dit_gemm_f16_kernel(const DitGemmArgs a) {
  static_assert(PRO == DIT_PRO_NONE || PRO == DIT_PRO_LN, "token Linears only");
  static_assert(EPI == DIT_EPI_BIAS || (WH && (EPI == DIT_EPI_GELU || EPI == DIT_EPI_GATE)), "the training step has the bias epilogue only");
  __shared__ __attribute__((aligned(16))) _Float16 As[GB * DH_S], Ws[GB * DH_S];
  __shared__ float s_mu[GB], s_rs[GB];
  __shared__ const float *s_mod[GB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long m0 = (long long)blockIdx.x * GB;
  const int n0 = blockIdx.y * GB;

  if (PRO == DIT_PRO_LN) {
    ln_tile_stats(a, m0, lane, wave, s_mu, s_rs, s_mod);
    __syncthreads();
  }

  dit_f32x16 acc;
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  const int wm = wave & 1, wn = wave >> 1;
  const int sr = tid >> 3, sk = (tid & 7) * 8;
  const float *arow[2], *wrow[2], *mrow[2];
  const _Float16 *whrow[2];
  float mu[2], rs[2];
  for (int h = 0; h < 2; ++h) {
    const long long r = m0 + sr + 32 * h;
    const int n = n0 + sr + 32 * h;
    arow[h] = r < a.M ? a.A + (a.a_compact ? r : phys_row(a, r)) * a.lda : nullptr;
    wrow[h] = !WH && n < a.N ? a.W + (long long)n * a.K : nullptr;
    whrow[h] = WH && n < a.N ? a.Wh + (long long)n * a.K : nullptr;
    mrow[h] = PRO == DIT_PRO_LN ? s_mod[sr + 32 * h] : nullptr;
    mu[h] = PRO == DIT_PRO_LN ? s_mu[sr + 32 * h] : 0.f;
    rs[h] = PRO == DIT_PRO_LN ? s_rs[sr + 32 * h] : 0.f;
  }
  // the chunk in flight: raw values in registers, fetched one chunk ahead so that the global loads run under the matrix
  // instructions of the chunk before; the prologue arithmetic and the rounding happen when they are stored to LDS
  float v[2][8], w[2][8], sc[2][8], sh[2][8];
  dit_f16x8 wh[2];
  auto fetch = [&](int k) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[h][e] = w[h][e] = sc[h][e] = sh[h][e] = 0.f;
      if (arow[h]) {
        dh_load8(arow[h], k, a.K, v[h]);
        if (PRO == DIT_PRO_LN) {
          dh_load8(mrow[h] + a.off_scale, k, a.K, sc[h]);
          dh_load8(mrow[h] + a.off_shift, k, a.K, sh[h]);
        }
      }
      if (WH) {
#pragma unroll
        for (int e = 0; e < 8; ++e) wh[h][e] = (_Float16)0.f;
        if (whrow[h] && k < a.K) wh[h] = *(const dit_f16x8 *)(whrow[h] + k);   // K % 8 == 0: the group ends at or before K
      } else if (wrow[h]) {
        dh_load8(wrow[h], k, a.K, w[h]);
      }
    }
  };
  fetch(sk);
  for (int k0 = 0; k0 < a.K; k0 += DH_K) {
    const int k = k0 + sk;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if (PRO == DIT_PRO_LN && arow[h]) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float xn = (v[h][e] - mu[h]) * rs[h];
          v[h][e] = k + e < a.K ? xn * (1.0f + sc[h][e]) + sh[h][e] : 0.f;   // modulate, DiT4D_V4.py:101-103
        }
      }
      *(dit_f16x8 *)(As + (sr + 32 * h) * DH_S + sk) = dh_round8(v[h]);
      *(dit_f16x8 *)(Ws + (sr + 32 * h) * DH_S + sk) = WH ? wh[h] : dh_round8(w[h]);
    }
    __syncthreads();
    if (k0 + DH_K < a.K) fetch(k + DH_K);
    acc = dh_mfma_chunk(As + (wm * 32 + (lane & 31)) * DH_S + 8 * (lane >> 5), Ws + (wn * 32 + (lane & 31)) * DH_S + 8 * (lane >> 5), acc);
    __syncthreads();
  }

  const int col = n0 + wn * 32 + (lane & 31);
  if (col >= a.N) return;
  const float bias = a.bias ? a.bias[col] : 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const long long rl = m0 + wm * 32 + (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
    if (rl >= a.M) continue;
    const long long prow = phys_row(a, rl);
    const float v = acc[i] + bias;
    if (EPI == DIT_EPI_BIAS) {
      a.Y[prow * a.ldy + col] = v;
    } else if (EPI == DIT_EPI_GELU) {
      a.Y[prow * a.ldy + col] = 0.5f * v * (1.0f + erff(v * 0.70710678118654752f));
    } else {   // DIT_EPI_GATE
      const float *mrow = a.mod + a.tbuf[prow / a.tok] * (long long)a.ldmod;
      float *y = a.Y + prow * a.ldy + col;
      *y = *y + mrow[a.off_gate + col] * v;
    }
  }
}

// Spatial self-attention: one 64-thread workgroup per (sample, slot, head); thread i = query token i (N_s <= 64).
// K / V of the head in LDS, scores of each query in its own LDS row, softmax and P V in fp32.
__global__ __launch_bounds__(64) void dit_attn_spatial_kernel(const DitAttnArgs a) {
  __shared__ float Ks[64 * 65], Vs[64 * 65], Ps[64 * 65];
  const int i = threadIdx.x;
  const int h = blockIdx.x % a.heads;
  const long long g = blockIdx.x / a.heads;                 // (sample, slot)
  const long long base = g * a.Ns;                          // first token row of the group
  const int E3 = 3 * a.E;
  for (int j = 0; j < a.Ns; ++j) {
    const float *row = a.qkv + (base + j) * E3 + h * 64;
    Ks[j * 65 + i] = row[a.E + i];
    Vs[j * 65 + i] = row[2 * a.E + i];
  }
  __syncthreads();
  if (i >= a.Ns) return;
  float q[64];
  const float *qr = a.qkv + (base + i) * E3 + h * 64;
#pragma unroll
  for (int d = 0; d < 64; ++d) q[d] = qr[d] * 0.125f;     // 1/sqrt(64), exact
  float mx = -INFINITY;
  for (int j = 0; j < a.Ns; ++j) {
    float s = 0.f;
#pragma unroll
    for (int d = 0; d < 64; ++d) s = fmaf(q[d], Ks[j * 65 + d], s);
    Ps[i * 65 + j] = s;
    mx = fmaxf(mx, s);
  }
  float den = 0.f;
  for (int j = 0; j < a.Ns; ++j) { const float e = expf(Ps[i * 65 + j] - mx); Ps[i * 65 + j] = e; den += e; }
  const float inv = 1.0f / den;
  float *o = a.out + (base + i) * a.E + h * 64;
  for (int d0 = 0; d0 < 64; d0 += 16) {
    float acc[16];
#pragma unroll
    for (int d = 0; d < 16; ++d) acc[d] = 0.f;
    for (int j = 0; j < a.Ns; ++j) {
      const float pj = Ps[i * 65 + j];
#pragma unroll
      for (int d = 0; d < 16; ++d) acc[d] = fmaf(pj, Vs[j * 65 + d0 + d], acc[d]);
    }
#pragma unroll
    for (int d = 0; d < 16; ++d) o[d0 + d] = acc[d] * inv;
  }
}

// Temporal cross-attention: one wave per (sample, patch, head), lane = head channel.  Keys / values: the T_p slots of
// the patch; queries: slots qs .. T_p-1 (DiT4D_V4.py:182-188).  Output rows are compact: [B][(T_p - qs) * N_s][E].
__global__ __launch_bounds__(256) void dit_attn_temporal_kernel(const DitAttnArgs a) {
  const int d = threadIdx.x & 63;
  const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const long long nw = (long long)a.B * a.Ns * a.heads;
  if (w >= nw) return;
  const int h = (int)(w % a.heads);
  const long long bp = w / a.heads;
  const int patch = (int)(bp % a.Ns);
  const long long b = bp / a.Ns;
  const int tok = a.Tp * a.Ns, nq = a.Tp - a.qs, E3 = 3 * a.E;
  const float *base = a.qkv + (b * tok + patch) * E3 + h * 64 + d;
  float k[TP_MAX], v[TP_MAX];
#pragma unroll
  for (int j = 0; j < TP_MAX; ++j) {
    k[j] = j < a.Tp ? base[(long long)j * a.Ns * E3 + a.E] : 0.f;
    v[j] = j < a.Tp ? base[(long long)j * a.Ns * E3 + 2 * a.E] : 0.f;
  }
  for (int qi = 0; qi < nq; ++qi) {
    const float q = base[(long long)(a.qs + qi) * a.Ns * E3] * 0.125f;
    float s[TP_MAX], mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < TP_MAX; ++j) {
      s[j] = wave_sum(q * k[j]);
      if (j < a.Tp) mx = fmaxf(mx, s[j]);
    }
    float den = 0.f, o = 0.f;
#pragma unroll
    for (int j = 0; j < TP_MAX; ++j)
      if (j < a.Tp) {
        const float e = expf(s[j] - mx);
        den += e;
        o = fmaf(e, v[j], o);
      }
    a.out[((b * nq + qi) * a.Ns + patch) * a.E + h * 64 + d] = o / den;
  }
}

// Full self-attention of DiT2D (DiT2D.py:105, 283-289): softmax(q k^T / 8) v over the S = T_p * N_s token rows of one
// (sample, head); one wave per 32-query tile, keys streamed in chunks of 32 with a running max and denominator, so no
// array bounds S.  Both products run on the exact-fp32 matrix instruction:
//   S^T = k q^T   A = k (row: key, k: head channel), B = q^T / 8: a lane's 16 accumulator values are 16 keys of ONE query
//                 (column = lane & 31), so the row max and sum are in-register plus one cross-half shuffle;
//   O^T = v^T P^T A = v^T (row: head channel, k: key), B = P^T: accumulator value r of a lane is key (r & 3) + 8 (r >> 2)
//                 + 4 (lane >> 5) of its query, which is exactly the B operand (k = lane >> 5) of a step that contracts
//                 that key pair -- P goes from the first product's registers into the second without a round trip, and
//                 the O^T columns are again one query per lane (the rescale by exp(m_old - m_new) is per lane).
// Tail keys (S is no multiple of 32: ATC has 216) get the score -inf, hence the weight exactly 0; their addresses and
// those of tail query rows are clamped to row S - 1 of the same sample and tail query rows are not stored.
__global__ __launch_bounds__(64) void dit_attn_full_kernel(const DitAttnArgs a) {
  const int lane = threadIdx.x, c = lane & 31, hf = lane >> 5;
  const int S = a.Tp * a.Ns, nqt = (S + 31) / 32, E3 = 3 * a.E;
  const int qt = blockIdx.x % nqt;
  const long long bh = blockIdx.x / nqt;
  const int h = (int)(bh % a.heads);
  const long long b = bh / a.heads;
  const float *base = a.qkv + b * S * E3 + h * 64;
  const int q = qt * 32 + c;
  float qv[32];   // q / 8 (exact) at the head channels 2 s + hf this lane feeds to step s
  {
    const float4 *qr = (const float4 *)(base + (long long)min(q, S - 1) * E3);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const float4 v = qr[i];
      qv[2 * i] = (hf ? v.y : v.x) * 0.125f;
      qv[2 * i + 1] = (hf ? v.w : v.z) * 0.125f;
    }
  }
  float m = -INFINITY, den = 0.f;
  dit_f32x16 o0, o1;
#pragma unroll
  for (int r = 0; r < 16; ++r) { o0[r] = 0.f; o1[r] = 0.f; }
  // Software pipeline: a chunk's V rows are requested before its q k^T chain and the next chunk's K row before its
  // softmax and P v chain, so that each load has 32 matrix instructions to land behind.
  float kc[32];   // the chunk's K operands, picked like qv
  auto load_k = [&](int k0) {
    const float4 *kr = (const float4 *)(base + a.E + (long long)min(k0 + c, S - 1) * E3);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const float4 v = kr[i];
      kc[2 * i] = hf ? v.y : v.x;
      kc[2 * i + 1] = hf ? v.w : v.z;
    }
  };
  load_k(0);
  const float *vb = base + 2 * a.E + c;
  for (int k0 = 0; k0 < S; k0 += 32) {
    float v0[16], v1[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float *vr = vb + (long long)min(k0 + (r & 3) + 8 * (r >> 2) + 4 * hf, S - 1) * E3;
      v0[r] = vr[0];
      v1[r] = vr[32];
    }
    dit_f32x16 s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
    for (int i = 0; i < 32; ++i) s = __builtin_amdgcn_mfma_f32_32x32x2f32(kc[i], qv[i], s, 0, 0, 0);
    load_k(k0 + 32);   // past the last chunk: row S - 1 again, never used
    float cmax = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      if (k0 + (r & 3) + 8 * (r >> 2) + 4 * hf >= S) s[r] = -INFINITY;
      cmax = fmaxf(cmax, s[r]);
    }
    cmax = fmaxf(cmax, __shfl_xor(cmax, 32, 64));
    const float mn = fmaxf(m, cmax);        // finite from the first chunk on: every chunk holds a key < S
    const float alpha = expf(m - mn);       // first chunk: exp(-inf) = 0
    float csum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) { s[r] = expf(s[r] - mn); csum += s[r]; }
    csum += __shfl_xor(csum, 32, 64);
    den = den * alpha + csum;
    m = mn;
#pragma unroll
    for (int r = 0; r < 16; ++r) { o0[r] *= alpha; o1[r] *= alpha; }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(v0[r], s[r], o0, 0, 0, 0);
      o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(v1[r], s[r], o1, 0, 0, 0);
    }
  }
  if (q >= S) return;
  // O^T: column = query, row = head channel (r & 3) + 8 (r >> 2) + 4 hf (+ 32 in o1): four consecutive channels per r >> 2
  float *orow = a.out + (b * S + q) * a.E + h * 64 + 4 * hf;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    *(float4 *)(orow + 8 * g) = make_float4(o0[4 * g] / den, o0[4 * g + 1] / den, o0[4 * g + 2] / den, o0[4 * g + 3] / den);
    *(float4 *)(orow + 32 + 8 * g) = make_float4(o1[4 * g] / den, o1[4 * g + 1] / den, o1[4 * g + 2] / den, o1[4 * g + 3] / den);
  }
}

// dit_attn_full_kernel on f16 operands (the f16a plan of an FM-DiT handle: cm_model_set_precision(CM_PRECISION_F16A)): the same
// streaming structure -- one wave per (sample, head, 32-query tile), keys in chunks of 32, running max and denominator in fp32, no
// array bounds S, one writer per output element, fixed order, no atomics, a sample reads only its own rows -- with both products
// on v_mfma_f32_32x32x16_f16 and fp32 accumulation (operand map: cm_dit_f16.h).
// Rounding (all fp32 -> f16 round-to-nearest-even, no clamp: a value past 65504 becomes +-inf and surfaces as a non-finite output):
// q * 0.125 is formed in fp32, then rounded; k and v are rounded when loaded; p = expf(s - m) is fp32, the denominator accumulates
// the UNROUNDED p, and p is rounded as the second product's operand; the rescale by exp(m_old - m_new) and the final o / den are fp32.
//   S^T = k q^T   A = k, B = q^T: four K = 16 steps over the 64 head channels; per step a lane supplies the eight channels
//                 16 s + 8 hf + j of its key row and of its query row (32 contiguous bytes each).  The accumulator map is the fp32
//                 instruction's: value r of a lane is key (r & 3) + 8 (r >> 2) + 4 hf of the chunk for the query lane & 31, so the
//                 row max and sum are in-register plus one cross-half shuffle, as in dit_attn_full_kernel.
//   O^T = v^T P^T two K = 16 steps over the chunk's 32 keys.  P goes from the accumulator registers straight into the B operand:
//                 registers 8 s .. 8 s + 7 are the fragment of step s, so element j of lane half hf is key
//                 16 s + 8 (j >> 2) + 4 hf + (j & 3) of the chunk -- NOT the natural 16 s + 8 hf + j.  A contraction is indifferent to
//                 the order of its k index as long as both operands agree, so the A operand v^T is gathered in that same permuted
//                 key order: these are the 16 rows (r & 3) + 8 (r >> 2) + 4 hf that dit_attn_full_kernel gathers.
// Tail keys get the score -inf (weight exactly 0) and a zero v operand; their addresses and those of tail query rows are clamped to
// row S - 1 of the same sample, and tail query rows are not stored.
__global__ __launch_bounds__(64) void dit_attn_full_f16_kernel(const DitAttnArgs a) {
  const int lane = threadIdx.x, c = lane & 31, hf = lane >> 5;
  const int S = a.Tp * a.Ns, nqt = (S + 31) / 32, E3 = 3 * a.E;
  const int qt = blockIdx.x % nqt;
  const long long bh = blockIdx.x / nqt;
  const int h = (int)(bh % a.heads);
  const long long b = bh / a.heads;
  const float *base = a.qkv + b * S * E3 + h * 64;
  const int q = qt * 32 + c;
  dit_f16x8 qh[4];   // round(q / 8) at the head channels 16 s + 8 hf + j this lane feeds to step s
  {
    const float *qr = base + (long long)min(q, S - 1) * E3 + 8 * hf;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const float4 x = *(const float4 *)(qr + 16 * s), y = *(const float4 *)(qr + 16 * s + 4);
      const float t[8] = {x.x * 0.125f, x.y * 0.125f, x.z * 0.125f, x.w * 0.125f, y.x * 0.125f, y.y * 0.125f, y.z * 0.125f, y.w * 0.125f};
      qh[s] = dh_round8(t);
    }
  }
  float m = -INFINITY, den = 0.f;
  dit_f32x16 o0, o1;
#pragma unroll
  for (int r = 0; r < 16; ++r) { o0[r] = 0.f; o1[r] = 0.f; }
  // Software pipeline as in dit_attn_full_kernel: a chunk's V rows are requested before its q k^T chain and the next chunk's K row
  // before its softmax and P v chain.  K is held raw (fp32) while in flight and rounded when it is fed to the matrix unit.
  float kc[4][8];   // the chunk's K operands, picked like qh
  auto load_k = [&](int k0) {
    const float *kr = base + a.E + (long long)min(k0 + c, S - 1) * E3 + 8 * hf;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const float4 x = *(const float4 *)(kr + 16 * s), y = *(const float4 *)(kr + 16 * s + 4);
      kc[s][0] = x.x; kc[s][1] = x.y; kc[s][2] = x.z; kc[s][3] = x.w; kc[s][4] = y.x; kc[s][5] = y.y; kc[s][6] = y.z; kc[s][7] = y.w;
    }
  };
  load_k(0);
  const float *vb = base + 2 * a.E + c;
  for (int k0 = 0; k0 < S; k0 += 32) {
    float v0[16], v1[16];   // v[key (r & 3) + 8 (r >> 2) + 4 hf][channel c | c + 32]: the permuted key order of the P fragments
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float *vr = vb + (long long)min(k0 + (r & 3) + 8 * (r >> 2) + 4 * hf, S - 1) * E3;
      v0[r] = vr[0];
      v1[r] = vr[32];
    }
    dit_f32x16 s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) s = __builtin_amdgcn_mfma_f32_32x32x16_f16(dh_round8(kc[i]), qh[i], s, 0, 0, 0);
    load_k(k0 + 32);   // past the last chunk: row S - 1 again, never used
    float cmax = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      if (k0 + (r & 3) + 8 * (r >> 2) + 4 * hf >= S) { s[r] = -INFINITY; v0[r] = 0.f; v1[r] = 0.f; }
      cmax = fmaxf(cmax, s[r]);
    }
    cmax = fmaxf(cmax, __shfl_xor(cmax, 32, 64));
    const float mn = fmaxf(m, cmax);        // finite from the first chunk on: every chunk holds a key < S
    const float alpha = expf(m - mn);       // first chunk: exp(-inf) = 0
    float csum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) { s[r] = expf(s[r] - mn); csum += s[r]; }   // the denominator takes the unrounded weights
    csum += __shfl_xor(csum, 32, 64);
    den = den * alpha + csum;
    m = mn;
#pragma unroll
    for (int r = 0; r < 16; ++r) { o0[r] *= alpha; o1[r] *= alpha; }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      dit_f16x8 p;
#pragma unroll
      for (int j = 0; j < 8; ++j) p[j] = (_Float16)s[8 * i + j];
      o0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(dh_round8(v0 + 8 * i), p, o0, 0, 0, 0);
      o1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(dh_round8(v1 + 8 * i), p, o1, 0, 0, 0);
    }
  }
  if (q >= S) return;
  // O^T: column = query, row = head channel (r & 3) + 8 (r >> 2) + 4 hf (+ 32 in o1): four consecutive channels per r >> 2
  float *orow = a.out + (b * S + q) * a.E + h * 64 + 4 * hf;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    *(float4 *)(orow + 8 * g) = make_float4(o0[4 * g] / den, o0[4 * g + 1] / den, o0[4 * g + 2] / den, o0[4 * g + 3] / den);
    *(float4 *)(orow + 32 + 8 * g) = make_float4(o1[4 * g] / den, o1[4 * g + 1] / den, o1[4 * g + 2] / den, o1[4 * g + 3] / den);
  }
}

}  // namespace

hipError_t launch_dit_gemm(const DitGemmArgs &a, hipStream_t st) {
  if (a.M <= 0) return hipSuccess;
  dim3 grid((unsigned)((a.M + GB - 1) / GB), (unsigned)((a.N + GB - 1) / GB));
  if (a.f16) {   // a missing f16 form is an error, never the fp32 kernel
#define CM_DIT_H(P, E, WH) \
  if (a.pro == P && a.epi == E && (a.Wh != nullptr) == WH) { hipLaunchKernelGGL((dit_gemm_f16_kernel<P, E, WH>), grid, dim3(256), 0, st, a); return hipGetLastError(); }
    CM_DIT_H(DIT_PRO_NONE, DIT_EPI_BIAS, false)   // the autocast training step: fp32 master weights
    CM_DIT_H(DIT_PRO_LN, DIT_EPI_BIAS, false)
    if (a.K % 8) return hipErrorInvalidValue;     // the f16 sampling plan: 16-byte groups of pre-rounded halves
    CM_DIT_H(DIT_PRO_LN, DIT_EPI_BIAS, true)
    CM_DIT_H(DIT_PRO_LN, DIT_EPI_GELU, true)
    CM_DIT_H(DIT_PRO_NONE, DIT_EPI_GATE, true)
#undef CM_DIT_H
    return hipErrorInvalidValue;
  }
#define CM_DIT_G(P, E) \
  if (a.pro == P && a.epi == E) { hipLaunchKernelGGL((dit_gemm_kernel<P, E>), grid, dim3(256), 0, st, a); return hipGetLastError(); }
  CM_DIT_G(DIT_PRO_NONE, DIT_EPI_BIAS)
  CM_DIT_G(DIT_PRO_NONE, DIT_EPI_SILU)
  CM_DIT_G(DIT_PRO_NONE, DIT_EPI_SILU2)
  CM_DIT_G(DIT_PRO_NONE, DIT_EPI_GATE)
  CM_DIT_G(DIT_PRO_LN, DIT_EPI_BIAS)
  CM_DIT_G(DIT_PRO_LN, DIT_EPI_GELU)
  CM_DIT_G(DIT_PRO_LN, DIT_EPI_UNPATCH)
  CM_DIT_G(DIT_PRO_PATCH, DIT_EPI_PATCH)
#undef CM_DIT_G
  return hipErrorInvalidValue;
}

hipError_t launch_dit_attn_spatial(const DitAttnArgs &a, hipStream_t st) {
  if (a.Ns < 1 || a.Ns > 64) return hipErrorInvalidValue;
  hipLaunchKernelGGL(dit_attn_spatial_kernel, dim3((unsigned)((long long)a.B * a.Tp * a.heads)), dim3(64), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_dit_attn_temporal(const DitAttnArgs &a, hipStream_t st) {
  if (a.Tp < 1 || a.Tp > TP_MAX || a.qs >= a.Tp) return hipErrorInvalidValue;
  const long long nw = (long long)a.B * a.Ns * a.heads;
  hipLaunchKernelGGL(dit_attn_temporal_kernel, dim3((unsigned)((nw + 3) / 4)), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_dit_attn_full(const DitAttnArgs &a, hipStream_t st) {
  const long long S = (long long)a.Tp * a.Ns;
  if (S < 1 || a.E != 64 * a.heads) return hipErrorInvalidValue;
  const long long nblk = (long long)a.B * a.heads * ((S + 31) / 32);
  if (nblk > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(dit_attn_full_kernel, dim3((unsigned)nblk), dim3(64), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_dit_attn_full_f16(const DitAttnArgs &a, hipStream_t st) {
  const long long S = (long long)a.Tp * a.Ns;
  if (S < 1 || a.E != 64 * a.heads) return hipErrorInvalidValue;
  const long long nblk = (long long)a.B * a.heads * ((S + 31) / 32);
  if (nblk > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(dit_attn_full_f16_kernel, dim3((unsigned)nblk), dim3(64), 0, st, a);
  return hipGetLastError();
}

}  // namespace cm
