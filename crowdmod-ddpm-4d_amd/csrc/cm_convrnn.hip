// ConvRNN forecaster kernels (reference: models/convRNN/{forecaster,encoder,convGRUCell,convLSTMCell}.py).  The host plan
// lives in cm_convrnn_host.inc.
//
// Activations are channels-last fp32 [B][H][W][C], C a multiple of 8.  One kernel carries the whole forecast (on the f16 plan its
// counterpart crnn_conv_f16_kernel, further down, carries every launch but the first and the last conv):
//   crnn_conv_kernel  Y = epilogue(conv(x0 || x1, W)) as an implicit GEMM on the exact-fp32 matrix instruction
//                     (v_mfma_f32_32x32x2_f32).  M = the pixels of ALL samples (the quarter-resolution level of the ATC
//                     grid has 27 pixels per sample, a 4 x 4 grid has one), N = output channels, K = taps * (C0 + C1) with
//                     k = tap * (C0 + C1) + c, so that eight consecutive k are eight consecutive channels of one tap of one
//                     source: the channel concat [x, h] of the cells is two base pointers, never a tensor.
//                     Geometries: 3x3 stride 1 pad 1; 3x3 stride 2 pad 1; ConvTranspose2d 4x4 stride 2 pad 1 as four
//                     output-parity classes (blockIdx.z) of 2x2 taps each: output (2 qy + py, 2 qx + px) reads input
//                     (qy + py - ty, qx + px - tx) through weight tap (1 - py + 2 ty, 1 - px + 2 tx).
//                     Epilogues: LeakyReLU(0.2); the GRU's r and u gates in one launch (N = 2 hid: writes r * h_prev and u);
//                     the GRU candidate (tanh, then h' = (1 - u) cand + u h_prev into the other buffer of the level's
//                     ping-pong pair: neighbouring pixels of this launch still read h_prev); the LSTM (N = 4 hid, packed
//                     column 4 ch + gate, so that the four gates of a channel are adjacent in the tile: c is updated in
//                     place, h' goes to the other buffer); the forecaster's last conv (frame t of the result in the
//                     reference layout, and the window frame the slide frees with exp on channels 0 and 3).
//                     The accumulator tile goes through LDS once, so that an epilogue sees whole pixel rows: stores are
//                     contiguous along channels and the LSTM's thread holds i, f, o, g of its channel.
// Determinism: every output element is written by one thread, k ascending (32-product chains summed in order), no atomics; a row of
// the GEMM reads only its own sample, so a result does not depend on the batch it ran in or on max_batch.
// Saturation: sigmoid is 1 / (1 + exp(-x)) (exp(-x) = inf gives 0) and tanh is tanhf: both are finite for any finite x.
#include "cm_kernels.h"
#include "cm_dit_f16.h"

#include <math.h>

namespace cm {

typedef float crnn_f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int TB = 64;       // rows and columns of a workgroup tile (2 x 2 waves of 32 x 32)
constexpr int TK = 32;       // k chunk staged in LDS
constexpr int TS = TK + 1;   // row stride of the staged operands
constexpr int CS = TB + 1;   // row stride of the accumulator tile (TB * CS <= 2 * TB * TS)

__device__ __forceinline__ float sigmoidf(float x) { return 1.0f / (1.0f + expf(-x)); }
// exp of the density and variance channels (forecaster.py:169-171, convRNN.py:228-229), rounded once from double
__device__ __forceinline__ float exp03(float v, int ch) { return (ch == 0 || ch == 3) ? (float)exp((double)v) : v; }

// The wave's 32 x 32 accumulator into the workgroup's tile Cs [TB][CS].  C/D map (the same for the fp32 and the f16 instruction):
// column = lane & 31, row = (i & 3) + 8 (i >> 2) + 4 (lane >> 5).
__device__ __forceinline__ void crnn_store_tile(float *Cs, const crnn_f32x16 &acc, int wm, int wn, int lane) {
#pragma unroll
  for (int i = 0; i < 16; ++i)
    Cs[(wm * 32 + (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5)) * CS + wn * 32 + (lane & 31)] = acc[i];
}

// The epilogue of a tile Cs [TB][CS] whose rows start at m0 and columns at n0, shared by crnn_conv_kernel and
// crnn_conv_f16_kernel: fp32 on either plan.
template <int GEO, int EPI>
__device__ __forceinline__ void crnn_epilogue(const CrnnConvArgs &a, const float *Cs, int tid, int m0, int n0, int M, int Hm, int Wm,
                                              int py, int px) {
  constexpr int CPR = EPI == CRNN_EPI_LSTM ? 16 : 64;   // outputs per tile row: the LSTM folds four columns into one channel
  for (int e = tid; e < TB * CPR; e += 256) {
    const int row = e / CPR, cl = e % CPR;
    const int rl = m0 + row;
    if (rl >= M) continue;
    const int eb = rl / (Hm * Wm), eq = rl % (Hm * Wm);
    const int oy = GEO == CRNN_GEO_T4 ? 2 * (eq / Wm) + py : eq / Wm, ox = GEO == CRNN_GEO_T4 ? 2 * (eq % Wm) + px : eq % Wm;
    const long long pix = ((long long)eb * a.Ho + oy) * a.Wo + ox;
    if (EPI == CRNN_EPI_LSTM) {
      const int hid = a.N >> 2, ch = (n0 >> 2) + cl;
      if (ch >= hid) continue;
      const float *g = Cs + row * CS + 4 * cl;   // i, f, o, g (convLSTMCell.py:62)
      const long long o = pix * hid + ch;
      const float gi = sigmoidf(g[0]), gf = sigmoidf(g[1]), go = sigmoidf(g[2]), gg = tanhf(g[3]);
      const float cn = gf * a.c[o] + gi * gg, tc = tanhf(cn);
      (a.cn ? a.cn : a.c)[o] = cn;
      a.y[o] = go * tc;
      if (a.t0) { *(float4 *)(a.t0 + pix * a.N + 4 * ch) = make_float4(gi, gf, go, gg); a.t1[o] = tc; }
      continue;
    }
    const int col = n0 + cl;
    if (col >= a.N) continue;
    const float v = Cs[row * CS + cl];
    if (EPI == CRNN_EPI_LEAKY) {
      a.y[pix * a.N + col] = v > 0.f ? v : 0.2f * v;
    } else if (EPI == CRNN_EPI_GRU_GATES) {   // columns [0, hid): reset gate, [hid, 2 hid): update gate
      const int hid = a.N >> 1;
      const float s = sigmoidf(v);
      if (col < hid) {
        a.y[pix * hid + col] = s * a.hprev[pix * hid + col];
        if (a.t0) a.t0[pix * hid + col] = s;
      } else a.u[pix * hid + col - hid] = s;
    } else if (EPI == CRNN_EPI_GRU_CAND) {    // convGRUCell.py:64-66
      const long long o = pix * a.N + col;
      const float uu = a.u[o], cand = tanhf(v);
      a.y[o] = (1.0f - uu) * cand + uu * a.hprev[o];
      if (a.t0) a.t0[o] = cand;
    } else {                                  // CRNN_EPI_LAST
      a.out[((((long long)eb * a.N + col) * a.Ho + oy) * a.Wo + ox) * a.Ft + a.t] = a.exp_out ? exp03(v, col) : v;
      if (a.win) a.win[(long long)eb * a.win_bs + ((long long)oy * a.Wo + ox) * 8 + col] = exp03(v, col);
    }
  }
}

template <int GEO, int EPI>
__global__ __launch_bounds__(256) void crnn_conv_kernel(const CrnnConvArgs a) {
  __shared__ float S[2 * TB * TS];
  float *As = S, *Ws = S + TB * TS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cls = GEO == CRNN_GEO_T4 ? (int)blockIdx.z : 0, py = cls >> 1, px = cls & 1;
  const int Hm = GEO == CRNN_GEO_T4 ? a.Hi : a.Ho, Wm = GEO == CRNN_GEO_T4 ? a.Wi : a.Wo;   // row grid of the GEMM
  const int M = a.B * Hm * Wm;
  const int m0 = blockIdx.x * TB, n0 = blockIdx.y * TB;
  const int Cin = a.C0 + a.C1, K = (GEO == CRNN_GEO_T4 ? 4 : 9) * Cin;
  const float *W = a.W + (long long)cls * a.N * K;

  crnn_f32x16 acc;
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  const int wm = wave & 1, wn = wave >> 1;
  const int sr = tid >> 2, sk = (tid & 3) * 8;   // staging: one row, eight consecutive k per thread
  const int r = m0 + sr, n = n0 + sr;
  const bool rok = r < M;
  const int b = rok ? r / (Hm * Wm) : 0, q = rok ? r % (Hm * Wm) : 0, qy = q / Wm, qx = q % Wm;
  const float *s0 = a.x0 + (long long)b * a.bs0;
  const float *s1 = a.x1 ? a.x1 + (long long)b * a.bs1 : nullptr;
  for (int k0 = 0; k0 < K; k0 += TK) {
    const int k = k0 + sk;
    float4 v0 = make_float4(0.f, 0.f, 0.f, 0.f), v1 = v0, w0 = v0, w1 = v0;
    if (k < K) {
      const int tap = k / Cin, c = k - tap * Cin;
      int iy, ix;
      if (GEO == CRNN_GEO_T4) {
        iy = qy + py - (tap >> 1); ix = qx + px - (tap & 1);
      } else {
        const int st = GEO == CRNN_GEO_S2 ? 2 : 1;
        iy = st * qy + tap / 3 - 1; ix = st * qx + tap % 3 - 1;
      }
      if (rok && iy >= 0 && iy < a.Hi && ix >= 0 && ix < a.Wi) {
        const long long pix = (long long)iy * a.Wi + ix;
        const float *p = c < a.C0 ? s0 + pix * a.C0 + c : s1 + pix * a.C1 + (c - a.C0);
        v0 = *(const float4 *)p; v1 = *(const float4 *)(p + 4);
      }
      if (n < a.N) {
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
    // two-level sum: a chunk's 32 products in one chain, then one add into the running sum -- the rounding error of a
    // K = 720 ... 4608 contraction grows like that of a blocked sum, not like one chain's (fixed order either way)
    crnn_f32x16 part;
#pragma unroll
    for (int i = 0; i < 16; ++i) part[i] = 0.f;
#pragma unroll
    for (int kk = 0; kk < TK; kk += 2) part = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[kk], bp[kk], part, 0, 0, 0);
    acc += part;
    __syncthreads();
  }

  float *Cs = S;   // the tile replaces the staged operands
  crnn_store_tile(Cs, acc, wm, wn, lane);
  __syncthreads();
  crnn_epilogue<GEO, EPI>(a, Cs, tid, m0, n0, M, Hm, Wm, py, px);
}

// The f16 plan's conv (cm_convrnn_set_precision(CM_PRECISION_F16)): the same implicit GEMM, tile, k order (k = tap * (C0 + C1) + c)
// and epilogues with the products on v_mfma_f32_32x32x16_f16.  Operands: the weights are a.Wh, rounded once on the host
// (cm_convrnn_finalize); an activation is rounded once, fp32 -> f16 round-to-nearest-even without a clamp, when it is staged
// (dh_round8): a source stays the fp32 tensor its producer wrote, so r * h_prev is the fp32 product, then rounded.  Sum: a
// chunk's DH_K = 64 products in one chain of four instructions, then one fp32 add into the running sum, k ascending.
// LDS: two buffers of the image cm_dit_f16.h documents (row stride 72 halves, ds_read_b128 operand reads, conflict-free), A then W.
// The global loads of chunk i + 1 are issued before the matrix instructions of chunk i and written to the other buffer after
// them: one barrier per chunk.  A thread stages row tid >> 2, k groups (tid & 3) * 8 and + 32: four lanes read 128 contiguous
// bytes of a source pixel (64 of a weight row).  Zero fill: rows >= M, columns >= N, k >= K, padding taps.
template <int GEO, int EPI>
__global__ __launch_bounds__(256) void crnn_conv_f16_kernel(const CrnnConvArgs a) {
  constexpr int IMG = TB * DH_S;                                  // halves of one operand image
  __shared__ __attribute__((aligned(16))) _Float16 S[4 * IMG];    // [2 buffers][A, W]; 36864 B >= the fp32 tile TB * CS * 4
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cls = GEO == CRNN_GEO_T4 ? (int)blockIdx.z : 0, py = cls >> 1, px = cls & 1;
  const int Hm = GEO == CRNN_GEO_T4 ? a.Hi : a.Ho, Wm = GEO == CRNN_GEO_T4 ? a.Wi : a.Wo;   // row grid of the GEMM
  const int M = a.B * Hm * Wm;
  const int m0 = blockIdx.x * TB, n0 = blockIdx.y * TB;
  const int Cin = a.C0 + a.C1, K = (GEO == CRNN_GEO_T4 ? 4 : 9) * Cin;
  const _Float16 *W = a.Wh + (long long)cls * a.N * K;

  crnn_f32x16 acc;
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  const int wm = wave & 1, wn = wave >> 1;
  const int sr = tid >> 2, sk = (tid & 3) * 8;
  const int r = m0 + sr, n = n0 + sr;
  const bool rok = r < M, nok = n < a.N;
  const int b = rok ? r / (Hm * Wm) : 0, q = rok ? r % (Hm * Wm) : 0, qy = q / Wm, qx = q % Wm;
  const float *s0 = a.x0 + (long long)b * a.bs0;
  const float *s1 = a.x1 ? a.x1 + (long long)b * a.bs1 : nullptr;
  const _Float16 *wrow = W + (long long)(nok ? n : 0) * K;

  float4 v[2][2];
  dit_f16x8 w[2];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      const int k = k0 + sk + 32 * g;
      v[g][0] = v[g][1] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int e = 0; e < 8; ++e) w[g][e] = (_Float16)0.f;
      if (k >= K) continue;
      const int tap = k / Cin, c = k - tap * Cin;
      int iy, ix;
      if (GEO == CRNN_GEO_T4) {
        iy = qy + py - (tap >> 1); ix = qx + px - (tap & 1);
      } else {
        const int st = GEO == CRNN_GEO_S2 ? 2 : 1;
        iy = st * qy + tap / 3 - 1; ix = st * qx + tap % 3 - 1;
      }
      if (rok && iy >= 0 && iy < a.Hi && ix >= 0 && ix < a.Wi) {
        const long long pix = (long long)iy * a.Wi + ix;
        const float *p = c < a.C0 ? s0 + pix * a.C0 + c : s1 + pix * a.C1 + (c - a.C0);
        v[g][0] = *(const float4 *)p; v[g][1] = *(const float4 *)(p + 4);
      }
      if (nok) w[g] = *(const dit_f16x8 *)(wrow + k);
    }
  };
  auto stage = [&](int buf) {
    _Float16 *ad = S + buf * 2 * IMG + sr * DH_S + sk, *wd = ad + IMG;
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      const float f[8] = {v[g][0].x, v[g][0].y, v[g][0].z, v[g][0].w, v[g][1].x, v[g][1].y, v[g][1].z, v[g][1].w};
      *(dit_f16x8 *)(ad + 32 * g) = dh_round8(f);
      *(dit_f16x8 *)(wd + 32 * g) = w[g];
    }
  };
  fetch(0);
  stage(0);
  __syncthreads();
  int buf = 0;
  for (int k0 = 0; k0 < K; k0 += DH_K, buf ^= 1) {
    const bool more = k0 + DH_K < K;
    if (more) fetch(k0 + DH_K);
    const _Float16 *ap = S + buf * 2 * IMG + (wm * 32 + (lane & 31)) * DH_S + 8 * (lane >> 5);
    const _Float16 *bp = S + buf * 2 * IMG + IMG + (wn * 32 + (lane & 31)) * DH_S + 8 * (lane >> 5);
    crnn_f32x16 part;
#pragma unroll
    for (int i = 0; i < 16; ++i) part[i] = 0.f;
    part = dh_mfma_chunk(ap, bp, part);
    acc += part;
    if (more) stage(buf ^ 1);   // last read a barrier ago
    __syncthreads();
  }

  float *Cs = (float *)S;   // the tile replaces the staged operands
  crnn_store_tile(Cs, acc, wm, wn, lane);
  __syncthreads();
  crnn_epilogue<GEO, EPI>(a, Cs, tid, m0, n0, M, Hm, Wm, py, px);
}

__global__ __launch_bounds__(256) void crnn_pack_frames_kernel(const float *src, float *win, int B, int H, int W, int L, int nslots,
                                                               int slot0) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x, HW = (long long)H * W;
  if (i >= (long long)B * L * HW) return;
  const int p = (int)(i % HW), l = (int)((i / HW) % L), b = (int)(i / (HW * L));
  float v[4];
  for (int c = 0; c < 4; ++c) v[c] = src[(((long long)b * 4 + c) * HW + p) * L + l];
  float4 *d = (float4 *)(win + (((long long)b * nslots + slot0 + l) * HW + p) * 8);
  d[0] = make_float4(v[0], v[1], v[2], v[3]);
  d[1] = make_float4(0.f, 0.f, 0.f, 0.f);
}

__global__ __launch_bounds__(256) void crnn_state_nchw_kernel(const float *src, float *dst, int B, int C, int hw) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)B * C * hw) return;
  const int p = (int)(i % hw), c = (int)((i / hw) % C), b = (int)(i / ((long long)hw * C));
  dst[i] = src[((long long)b * hw + p) * C + c];
}

}  // namespace

hipError_t launch_crnn_conv(const CrnnConvArgs &a, hipStream_t st) {
  const bool t4 = a.geo == CRNN_GEO_T4;
  const long long M = (long long)a.B * (t4 ? a.Hi : a.Ho) * (t4 ? a.Wi : a.Wo);
  if (M <= 0) return hipSuccess;
  if (M > 0x7fffffffLL - TB || a.C0 < 8 || a.C0 % 8 || a.C1 < 0 || a.C1 % 8 || (a.C1 > 0) != (a.x1 != nullptr) || a.N < 1)
    return hipErrorInvalidValue;
  if ((a.epi == CRNN_EPI_LSTM && a.N % 4) || (a.epi == CRNN_EPI_GRU_GATES && a.N % 2) || (a.epi == CRNN_EPI_LAST && a.N > 8))
    return hipErrorInvalidValue;
  const int so = a.geo == CRNN_GEO_S1 ? 0 : 1;   // the output grid the geometry implies
  if (t4 ? (a.Ho != 2 * a.Hi || a.Wo != 2 * a.Wi) : (a.Ho != (a.Hi + so) / (so + 1) || a.Wo != (a.Wi + so) / (so + 1)))
    return hipErrorInvalidValue;
  dim3 grid((unsigned)((M + TB - 1) / TB), (unsigned)((a.N + TB - 1) / TB), t4 ? 4 : 1);
  if (a.Wh) {
#define CM_CRNN16(G, E) \
  if (a.geo == G && a.epi == E) { hipLaunchKernelGGL((crnn_conv_f16_kernel<G, E>), grid, dim3(256), 0, st, a); return hipGetLastError(); }
    CM_CRNN16(CRNN_GEO_S1, CRNN_EPI_LEAKY)
    CM_CRNN16(CRNN_GEO_S1, CRNN_EPI_GRU_GATES)
    CM_CRNN16(CRNN_GEO_S1, CRNN_EPI_GRU_CAND)
    CM_CRNN16(CRNN_GEO_S1, CRNN_EPI_LSTM)
    CM_CRNN16(CRNN_GEO_S2, CRNN_EPI_LEAKY)
    CM_CRNN16(CRNN_GEO_T4, CRNN_EPI_LEAKY)
#undef CM_CRNN16
    return hipErrorInvalidValue;   // no f16 form of this launch: never a quiet fp32 one
  }
#define CM_CRNN(G, E) \
  if (a.geo == G && a.epi == E) { hipLaunchKernelGGL((crnn_conv_kernel<G, E>), grid, dim3(256), 0, st, a); return hipGetLastError(); }
  CM_CRNN(CRNN_GEO_S1, CRNN_EPI_LEAKY)
  CM_CRNN(CRNN_GEO_S1, CRNN_EPI_GRU_GATES)
  CM_CRNN(CRNN_GEO_S1, CRNN_EPI_GRU_CAND)
  CM_CRNN(CRNN_GEO_S1, CRNN_EPI_LSTM)
  CM_CRNN(CRNN_GEO_S1, CRNN_EPI_LAST)
  CM_CRNN(CRNN_GEO_S2, CRNN_EPI_LEAKY)
  CM_CRNN(CRNN_GEO_T4, CRNN_EPI_LEAKY)
#undef CM_CRNN
  return hipErrorInvalidValue;
}

hipError_t launch_crnn_pack_frames(const float *src, float *win, int B, int H, int W, int L, int nslots, int slot0, hipStream_t st) {
  const long long n = (long long)B * L * H * W;
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(crnn_pack_frames_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, src, win, B, H, W, L, nslots, slot0);
  return hipGetLastError();
}

hipError_t launch_crnn_state_nchw(const float *src, float *dst, int B, int C, int h, int w, hipStream_t st) {
  const long long n = (long long)B * C * h * w;
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(crnn_state_nchw_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, src, dst, B, C, h * w);
  return hipGetLastError();
}

}  // namespace cm
