// Fused AttentionBlock (reference: /root/reference/models/backbones/layers.py:5-18):
//     x + MHA(GroupNorm(8, E)(x))          over S = Z*Y*X tokens, E channels, 4 heads of D = E/4
// as ONE launch per (head, sample) plus the K-split combine pass, instead of the five launches of the
// generic plan (GroupNorm finalise, in-projection conv, attention core, out-projection conv + the
// finalise in front of it).  At 54-216 tokens per sample these launches are latency chains: the whole
// block is 0.8 % of the UNet's FLOPs.
//
// One 768-thread workgroup = (head h, sample b) -- 12 waves, because LDS admits one workgroup per CU and every
// phase is a latency chain at one wave per SIMD:
//   1. x[b] (S x E, channels-last) -> LDS; GroupNorm statistics of all 8 groups straight from that copy
//      (two passes, fixed reduction order), normalised in place with the affine folded in;
//      the head's weight slices (3D rows of W_in, D columns of W_out) ride in the same single round of global
//      loads -- the kernel never waits on global memory again;
//   2. [q|k|v]_h = xn * W_in[h-slices]^T + b_in on the matrix cores (v_mfma_f32_16x16x4_f32, exact fp32):
//      wave w owns the 16-row blocks w, w+4, ...; both operands come from LDS rows in the REFERENCE weight
//      layout (a lane reads 16 contiguous bytes of one row: with the k values of an MFMA chosen as
//      {16j + 4*kq + jj} both fragments are plain float4 reads, no packing); q is pre-scaled by 1/sqrt(D);
//   3. softmax(q k^T) v per query row on the vector ALUs (online softmax, K / V rows broadcast from LDS),
//      written over q;
//   4. partial out-projection  y_h = o_h * W_out[:, h*D:(h+1)*D]^T  (S x E) on the matrix cores into
//      part[h][b]; ksplit_combine_kernel then sums the heads in a fixed order, adds the out-proj bias
//      and the residual x and emits the GroupNorm statistics of the result (cm_misc.hip).
// Nothing is reduced with atomics; sample b never touches another sample's data, so a chain's result
// does not depend on the batch it runs in.
//
// Where a sample has at most 64 tokens the default plan's inference forward takes attn_sample_kernel instead (second half of
// this file): the sample is the workgroup, so the head sum, bias, residual and statistics join the one launch.
#include "cm_kernels.h"

#include <algorithm>
#include <atomic>

namespace cm {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int ATT_NT = 768;                  // 12 waves, 3 per SIMD: one workgroup per CU (LDS), so latency hiding comes from here
constexpr int ATT_KS = 3;                    // key slices of the softmax phase (each query row: PARTS x KS lanes)

template <int D>
__global__ __launch_bounds__(ATT_NT) void attn_head_kernel(const AttnBlockArgs a) {
  constexpr int NT = ATT_NT, NW = NT / 64;
  constexpr int KD = D < 16 ? 16 : D;        // head dim padded to one 16-wide k chunk (zeros beyond D)
  constexpr int DS = KD + 4;                 // LDS row stride of q / k / v and of the out-projection slice
  constexpr int NBQ = (D + 15) / 16;         // 16-column blocks per q / k / v
  constexpr int NBT = 3 * NBQ;
  constexpr int PARTS = D / 8;               // lanes per (query row, key slice) in the softmax phase (8 dims each)
  constexpr int E = 4 * D;                   // nn.MultiheadAttention(E, 4 heads), layers.py:10 (checked on the host)
  constexpr int XS = E + 8;                  // LDS row stride of x / W_in rows: conflict-free ds_read_b128 fragments
  constexpr int Q4 = E >> 2;                 // channel quads (= D); NT % Q4 == 0
  constexpr int RL = NT / Q4;                // row lanes
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int S = a.S;
  float *Xs = sm;                            // [S][XS]
  float *Wi = Xs + (size_t)S * XS;           // [NBT * 16][XS]  in-projection rows of this head (q | k | v)
  float *Wo = Wi + (size_t)NBT * 16 * XS;    // [E][DS]         out-projection columns of this head
  float *Qs = Wo + (size_t)E * DS;           // [S][DS]   (later: the attention output o_h)
  float *Ks = Qs + (size_t)S * DS;
  float *Vs = Ks + (size_t)S * DS;
  float *bi = Vs + (size_t)S * DS;           // [NBT * 16] in-projection bias of this head
  float *red = bi + NBT * 16;                // [RL * 8] row-lane partials + [8] group totals
  const int h = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r16 = lane & 15, kq = lane >> 4;

  // ---- 0. ONE round of global loads: x[b], the head's weight slices, the affine -----------
  // A dependent global load costs 1.5-2 us under load on this part (profiles/round1_notes.md), so every load of
  // the kernel is issued here, back to back into registers (branch-free: clamped addresses), before the first
  // LDS store waits for any of them; nothing below this block touches global memory until the final stores.
  const int q4 = tid % Q4, rl = tid / Q4;
  const float *xb = a.x + (size_t)b * S * E;
  constexpr int UX = 3;                                    // x rows per thread and batch
  constexpr int NWI = (NBT * 16 + RL - 1) / RL;            // W_in rows per thread
  constexpr int NWO = (E * (KD / 4) + NT - 1) / NT;        // W_out float4 per thread
  f32x4 vx[UX], vwi[NWI], vwo[NWO];
#pragma unroll
  for (int u = 0; u < UX; ++u) vx[u] = *reinterpret_cast<const f32x4 *>(xb + (size_t)min(rl + u * RL, S - 1) * E + 4 * q4);
#pragma unroll
  for (int u = 0; u < NWI; ++u) {
    const int wr = min(rl + u * RL, NBT * 16 - 1);
    const int which = wr / (NBQ * 16), c = min(wr % (NBQ * 16), D - 1);   // rows beyond D of a padded block: any valid row
    vwi[u] = *reinterpret_cast<const f32x4 *>(a.w_in + (size_t)(which * E + h * D + c) * E + 4 * q4);
  }
#pragma unroll
  for (int u = 0; u < NWO; ++u) {
    const int i = min(tid + u * NT, E * (KD / 4) - 1);
    const int n = i / (KD / 4), c4 = min(i % (KD / 4), D / 4 - 1);
    vwo[u] = *reinterpret_cast<const f32x4 *>(a.w_out + (size_t)n * E + h * D + 4 * c4);
  }
  const f32x4 ga = *reinterpret_cast<const f32x4 *>(a.gamma + 4 * q4);
  const f32x4 be = *reinterpret_cast<const f32x4 *>(a.beta + 4 * q4);
  float bval = 0.f;
  {
    const int tb = min(tid, NBT * 16 - 1);
    const int which = tb / (NBQ * 16), c = min(tb % (NBQ * 16), D - 1);
    bval = a.b_in[which * E + h * D + c];
  }
  float s1 = 0.f;
#pragma unroll
  for (int u = 0; u < UX; ++u) {
    const int row = rl + u * RL;
    if (row < S) {
      *reinterpret_cast<f32x4 *>(Xs + row * XS + 4 * q4) = vx[u];
      s1 += (vx[u][0] + vx[u][1]) + (vx[u][2] + vx[u][3]);
    }
  }
#pragma unroll
  for (int u = 0; u < NWI; ++u) {
    const int wr = rl + u * RL;
    if (wr < NBT * 16) *reinterpret_cast<f32x4 *>(Wi + wr * XS + 4 * q4) = vwi[u];
  }
#pragma unroll
  for (int u = 0; u < NWO; ++u) {
    const int i = tid + u * NT;
    if (i < E * (KD / 4)) {
      const int n = i / (KD / 4), c4 = i % (KD / 4);
      *reinterpret_cast<f32x4 *>(Wo + n * DS + 4 * c4) = (4 * c4 < D) ? vwo[u] : f32x4{0.f, 0.f, 0.f, 0.f};   // zero beyond D
    }
  }
  if (tid < NBT * 16) bi[tid] = bval;
  for (int row0 = UX * RL; row0 < S; row0 += UX * RL) {   // samples with more than UX * RL tokens: further batches
#pragma unroll
    for (int u = 0; u < UX; ++u) vx[u] = *reinterpret_cast<const f32x4 *>(xb + (size_t)min(row0 + rl + u * RL, S - 1) * E + 4 * q4);
#pragma unroll
    for (int u = 0; u < UX; ++u) {
      const int row = row0 + rl + u * RL;
      if (row < S) {
        *reinterpret_cast<f32x4 *>(Xs + row * XS + 4 * q4) = vx[u];
        s1 += (vx[u][0] + vx[u][1]) + (vx[u][2] + vx[u][3]);
      }
    }
  }

  // ---- 1. GroupNorm of x[b] from the LDS copy (two passes, fixed reduction order) -------------
  constexpr int QPG = Q4 / 8;                // quads per group (GroupNorm(8, E): E/8 channels = D/8 quads... x4 heads)
  const int grp = q4 / QPG;
  auto group_sum = [&](float v) -> float {   // returns the group total to every thread
    // the QPG quads of a group sit in adjacent lanes of one wave: fold them first, then the RL row lanes
#pragma unroll
    for (int mk = 1; mk < QPG; mk <<= 1) v += __shfl_xor(v, mk);
    __syncthreads();
    if ((q4 & (QPG - 1)) == 0) red[rl * 8 + grp] = v;
    __syncthreads();
    if (tid < 8) {
      float t = 0.f;
      for (int r = 0; r < RL; ++r) t += red[r * 8 + tid];
      red[RL * 8 + tid] = t;
    }
    __syncthreads();
    return red[RL * 8 + grp];
  };
  const float cnt = (float)(E / 8) * (float)S;
  const float mean = group_sum(s1) / cnt;
  float s2 = 0.f;
  for (int row = rl; row < S; row += RL) {
    const f32x4 v = *reinterpret_cast<const f32x4 *>(Xs + row * XS + 4 * q4);
    const float d0 = v[0] - mean, d1 = v[1] - mean, d2 = v[2] - mean, d3 = v[3] - mean;
    s2 += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
  }
  const float rstd = rsqrtf(group_sum(s2) / cnt + a.eps);   // biased variance, layers.py:9 (nn.GroupNorm)
  {
    const f32x4 sc = ga * rstd;
    const f32x4 sh = be - sc * mean;
    for (int row = rl; row < S; row += RL) {
      f32x4 *p = reinterpret_cast<f32x4 *>(Xs + row * XS + 4 * q4);
      *p = *p * sc + sh;
    }
  }
  __syncthreads();

  // ---- 2. q, k, v of this head: one 16 x 16 output block per wave and round -------------------
  const int nmb = (S + 15) >> 4;
  constexpr int nj = E >> 4;                 // 16-wide k chunks of the in-projection
  const float qscale = rsqrtf((float)D);
  for (int item = wave; item < nmb * NBT; item += NW) {
    const int mb = item / NBT, nb = item - mb * NBT;
    const int arow = min(mb * 16 + r16, S - 1);
    const float *ap = Xs + arow * XS + 4 * kq;
    const float *bp = Wi + (nb * 16 + r16) * XS + 4 * kq;
    f32x4 af[nj], bf[nj];
#pragma unroll
    for (int j = 0; j < nj; ++j) {
      af[j] = *reinterpret_cast<const f32x4 *>(ap + 16 * j);
      bf[j] = *reinterpret_cast<const f32x4 *>(bp + 16 * j);
    }
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < nj; ++j)
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(af[j][jj], bf[j][jj], acc, 0, 0, 0);
    const int which = nb / NBQ, c = (nb % NBQ) * 16 + r16;
    float *dst = which == 0 ? Qs : (which == 1 ? Ks : Vs);
    const float bias = bi[nb * 16 + r16];
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int row = mb * 16 + 4 * kq + reg;
      float v = acc[reg] + bias;
      if (which == 0) v *= qscale;
      if (c >= D) v = 0.f;                    // padding columns of the k chunk (D < 16)
      if (row < S) dst[row * DS + c] = v;
    }
  }
  __syncthreads();

  // ---- 3. softmax(q k^T) v: a query row = PARTS lanes x ATT_KS key slices, merged in slice order ------
  {
    constexpr int LPR = PARTS * ATT_KS;       // lanes per query row
    constexpr int ROWS = NT / LPR;
    float *mrg = Xs;                          // x and W_in are dead: [min(S, ROWS)][KS][PARTS][12] merge scratch (m, l, -, -, o[8])
    const int part = tid % PARTS, ksl = (tid / PARTS) % ATT_KS, prow = tid / LPR;
    const int kper = (S + ATT_KS - 1) / ATT_KS;
    const int k0 = ksl * kper, k1 = min(S, k0 + kper);
    for (int row0 = 0; row0 < S; row0 += ROWS) {
      const int row = row0 + prow;
      const int rowc = row < S ? row : S - 1;  // surplus lanes shadow the last row (shuffles stay convergent)
      const f32x4 q0 = *reinterpret_cast<const f32x4 *>(Qs + rowc * DS + 8 * part);
      const f32x4 q1 = *reinterpret_cast<const f32x4 *>(Qs + rowc * DS + 8 * part + 4);
      f32x4 o0 = {0.f, 0.f, 0.f, 0.f}, o1 = {0.f, 0.f, 0.f, 0.f};
      float mx = -3.0e38f, l = 0.f;
      for (int j = k0; j < k1; ++j) {
        const f32x4 kv0 = *reinterpret_cast<const f32x4 *>(Ks + j * DS + 8 * part);
        const f32x4 kv1 = *reinterpret_cast<const f32x4 *>(Ks + j * DS + 8 * part + 4);
        // two independent half-sums: half the dependent-FMA chain of a single accumulator
        float sa = q0[0] * kv0[0], sb = q1[0] * kv1[0];
        sa = fmaf(q0[1], kv0[1], sa); sb = fmaf(q1[1], kv1[1], sb);
        sa = fmaf(q0[2], kv0[2], sa); sb = fmaf(q1[2], kv1[2], sb);
        sa = fmaf(q0[3], kv0[3], sa); sb = fmaf(q1[3], kv1[3], sb);
        float sc = sa + sb;
#pragma unroll
        for (int m = 1; m < PARTS; m <<= 1) sc += __shfl_xor(sc, m);
        const f32x4 v0 = *reinterpret_cast<const f32x4 *>(Vs + j * DS + 8 * part);
        const f32x4 v1 = *reinterpret_cast<const f32x4 *>(Vs + j * DS + 8 * part + 4);
        if (sc > mx) {
          const float corr = __expf(mx - sc);
          l *= corr;
          o0 *= corr;
          o1 *= corr;
          mx = sc;
        }
        const float p = __expf(sc - mx);
        l += p;
        o0 += v0 * p;
        o1 += v1 * p;
      }
      // merge the key slices of a row in slice order (every q row of this pass has been read by now)
      __syncthreads();
      if (row < S) {
        float *mp = mrg + ((prow * ATT_KS + ksl) * PARTS + part) * 12;
        mp[0] = mx; mp[1] = l;
        *reinterpret_cast<f32x4 *>(mp + 4) = o0;
        *reinterpret_cast<f32x4 *>(mp + 8) = o1;
      }
      __syncthreads();
      if (ksl == 0 && row < S) {
        float M = -3.0e38f;
#pragma unroll
        for (int s2i = 0; s2i < ATT_KS; ++s2i) M = fmaxf(M, mrg[((prow * ATT_KS + s2i) * PARTS + part) * 12]);
        float L = 0.f;
        f32x4 O0 = {0.f, 0.f, 0.f, 0.f}, O1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s2i = 0; s2i < ATT_KS; ++s2i) {
          const float *mp = mrg + ((prow * ATT_KS + s2i) * PARTS + part) * 12;
          const float w = (mp[1] > 0.f) ? __expf(mp[0] - M) : 0.f;   // an empty slice (l = 0) contributes nothing
          L += mp[1] * w;
          O0 += *reinterpret_cast<const f32x4 *>(mp + 4) * w;
          O1 += *reinterpret_cast<const f32x4 *>(mp + 8) * w;
        }
        const float inv = 1.0f / L;
        *reinterpret_cast<f32x4 *>(Qs + row * DS + 8 * part) = O0 * inv;
        *reinterpret_cast<f32x4 *>(Qs + row * DS + 8 * part + 4) = O1 * inv;
      }
      __syncthreads();
    }
  }

  // ---- 4. partial out-projection of this head: one 16 x 16 block per wave and round -------------------
  {
    constexpr int NJ = KD / 16;
    constexpr int nbe = E >> 4;              // 16-column blocks of the output
    float *pout = a.part + ((size_t)h * a.B + b) * (size_t)S * E;
    for (int item = wave; item < nmb * nbe; item += NW) {
      const int mb = item / nbe, nb = item - mb * nbe;
      const int arow = min(mb * 16 + r16, S - 1);
      f32x4 af[NJ], bf[NJ];
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        af[j] = *reinterpret_cast<const f32x4 *>(Qs + arow * DS + 16 * j + 4 * kq);
        bf[j] = *reinterpret_cast<const f32x4 *>(Wo + (nb * 16 + r16) * DS + 16 * j + 4 * kq);
      }
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(af[j][jj], bf[j][jj], acc, 0, 0, 0);
      const int n = nb * 16 + r16;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int row = mb * 16 + 4 * kq + reg;
        if (row < S) pout[(size_t)row * E + n] = acc[reg];
      }
    }
  }
}

size_t attn_block_lds_bytes(int S, int E, int heads) {
  const int D = E / heads, KD = D < 16 ? 16 : D, NBT = 3 * ((D + 15) / 16);
  // (the softmax merge scratch, S * (D/8) * ATT_KS * 12 floats, overlays x and W_in, which are dead by then)
  return ((size_t)S * (E + 8) + (size_t)NBT * 16 * (E + 8) + (size_t)E * (KD + 4) + (size_t)3 * S * (KD + 4) + (size_t)NBT * 16 +
          (size_t)(ATT_NT / (E / 4)) * 8 + 8) * sizeof(float);
}

bool attn_block_ok(int S, int E, int heads, int groups) {
  if (heads != 4 || E % heads) return false;                      // the kernel's E = 4 * D is a compile-time constant
  const int D = E / heads;
  if (D != 8 && D != 16 && D != 32) return false;
  if (groups != 8 || E % (4 * groups)) return false;              // group = whole channel quads, 8 statistics lanes
  return S >= 1 && attn_block_lds_bytes(S, E, heads) <= 160 * 1024;
}

hipError_t launch_attn_block(const AttnBlockArgs &a, hipStream_t st) {
  if (!attn_block_ok(a.S, a.E, a.heads, a.groups)) return hipErrorInvalidValue;
  const int D = a.E / a.heads;
  const size_t smem = attn_block_lds_bytes(a.S, a.E, a.heads);
#define CM_ATTNB(DD)                                                                                        \
  if (D == DD) {                                                                                            \
    static bool attr_set[64] = {false};                                                                     \
    int dev = 0;                                                                                            \
    (void)hipGetDevice(&dev);                                                                               \
    if (!attr_set[dev & 63]) {                                                                              \
      hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(attn_head_kernel<DD>),              \
                                         hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);           \
      if (e != hipSuccess) return e;                                                                        \
      attr_set[dev & 63] = true;                                                                            \
    }                                                                                                       \
    hipLaunchKernelGGL((attn_head_kernel<DD>), dim3(a.heads, a.B), dim3(ATT_NT), smem, st, a);                 \
    return hipGetLastError();                                                                               \
  }
  CM_ATTNB(8) CM_ATTNB(16) CM_ATTNB(32)
#undef CM_ATTNB
  return hipErrorInvalidValue;
}


// --------------------------------------------------------------------------------
// The whole block as ONE launch: workgroup = sample, 1024 threads = 16 waves, four per head.  E = 128, D = 32, S <= 64.
//   0. one round of global loads: x[b] (two rows x one channel quad per thread; read again as the residual behind the in-projection), the affine,
//      two of the wave's three in-projection weight blocks;
//   1. GroupNorm statistics from the registers (two passes, fixed order: a group's quads and the wave's two row lanes by shuffle,
//      the 16 waves through LDS);
//   2. xn * 2^k as f16 (hi, mid) planes in LDS, k from the exact max |xn| of the sample (max * 2^k in [8192, 16384)); rows >= S zero;
//   3. [q|k|v] = xn W_in^T on v_mfma_f32_16x16x32_f16, three cross terms: a wave owns three 16-column blocks (their fragments come
//      from global memory once: two blocks with the first loads, the third while the second runs) and every
//      second 16-row block; accumulators * 2^-k (exact), + bias, q / sqrt(D); fp32 to LDS;
//   4. per (head, 16 queries) one wave: S^T = K Q^T and O^T = V^T P^T on v_mfma_f32_16x16x4_f32 -- in the accumulator layout a lane
//      owns one query and its registers are keys, so the softmax is lane-local plus two xor exchanges and the probabilities already
//      are the B operand of the second product (attn_core_f16_kernel, cm_misc.hip); keys >= S masked;
//   5. o * 2^k' as f16 (hi, mid) planes over xn's (k' from the exact max |o| of the sample), out-projection as in 3., to LDS;
//   6. + bias + residual, stores (the thread mapping of the loads), then the slot statistics of the result per channel in the format
//      of ksplit_combine_kernel: mean and M2 about it over the slot's rows, fixed order.
// A non-finite value in a sample reaches the matrix products as itself (inf splits into inf and NaN): the output is non-finite.
// --------------------------------------------------------------------------------
typedef _Float16 f16x8a __attribute__((ext_vector_type(8)));
typedef unsigned u32x4a __attribute__((ext_vector_type(4)));

constexpr int AS_NT = 1024, AS_E = 128, AS_D = 32, AS_SMAX = 64;
constexpr int AS_HS = AS_E + 8;              // row stride of an f16 plane in halves (272 B: 16-byte aligned, conflict-free b128 reads)
constexpr int AS_QS = AS_E + 4;              // row stride of q / k / v / y in floats
constexpr int AS_RED = 512;                  // reduction scratch in floats

size_t attn_sample_lds_bytes() {
  return (size_t)2 * AS_SMAX * AS_HS * sizeof(_Float16) + ((size_t)3 * AS_SMAX * AS_QS + AS_RED) * sizeof(float);
}

bool attn_sample_ok(int S, int E, int heads, int groups) { return E == AS_E && heads == 4 && groups == 8 && S >= 1 && S <= AS_SMAX; }

// power of two s with m s in [2^13, 2^14) for a finite m > 0 (1 otherwise), and its inverse: both exact
__device__ __forceinline__ float as_range_scale(float m, float *inv) {
  const unsigned e = (__float_as_uint(m) >> 23) & 255u;       // 2^(e - 127) <= m < 2^(e - 126)
  int se = 267 - (int)e;                                      // biased exponent of 2^(140 - e)
  se = se < 32 ? 32 : (se > 222 ? 222 : se);
  if (!(m > 0.f) || e == 255u) se = 127;
  *inv = __uint_as_float((unsigned)(254 - se) << 23);
  return __uint_as_float((unsigned)se << 23);
}

__global__ __launch_bounds__(AS_NT) void attn_sample_kernel(const AttnSampleArgs a) {
  constexpr int E = AS_E, D = AS_D, HS = AS_HS, QS = AS_QS, NT = AS_NT;
  extern __shared__ __attribute__((aligned(16))) unsigned char smraw[];
  _Float16 *XH = reinterpret_cast<_Float16 *>(smraw);          // [64][HS] hi terms of xn (later: of o)
  _Float16 *XM = XH + AS_SMAX * HS;                            // [64][HS] mid terms
  float *Qs = reinterpret_cast<float *>(XM + AS_SMAX * HS);    // [64][QS] (later: the out-projection y)
  float *Ks = Qs + AS_SMAX * QS;
  float *Vs = Ks + AS_SMAX * QS;
  float *red = Vs + AS_SMAX * QS;                              // two [16 waves][8 groups] partial sets, wave maxima at 272 / 288
  const int S = a.S, b = blockIdx.x, tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r16 = lane & 15, g4 = lane >> 4;
  const int nrb = (S + 15) >> 4;                               // 16-row blocks that hold a token

  // ---- 0. one round of global loads ------------------------------------------------------------------
  const int q4 = tid & 31, rl = tid >> 5;                      // channel quad, row lane: rows rl and rl + 32
  const float *xb = a.x + (size_t)b * S * E;
  f32x4 vx[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) vx[u] = *reinterpret_cast<const f32x4 *>(xb + (size_t)min(rl + 32 * u, S - 1) * E + 4 * q4);
  const f32x4 ga = *reinterpret_cast<const f32x4 *>(a.gamma + 4 * q4);
  const f32x4 be = *reinterpret_cast<const f32x4 *>(a.beta + 4 * q4);
  const int cb0 = 3 * (wave >> 1), rbp = wave & 1;             // in-projection: column blocks cb0 .. cb0 + 2, row blocks rbp, rbp + 2
  const u32x4a *wing = reinterpret_cast<const u32x4a *>(a.win_h2);
  u32x4a wf[3][4][2];                                          // the wave's fragments [column block][k step][hi, mid]
  float bias[3];
#pragma unroll
  for (int ci = 0; ci < 2; ++ci) {                             // two blocks now, the third once the GroupNorm's registers are free
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
#pragma unroll
      for (int t = 0; t < 2; ++t) wf[ci][ks][t] = wing[(((size_t)(cb0 + ci) * 4 + ks) * 2 + t) * 64 + lane];
  }
#pragma unroll
  for (int ci = 0; ci < 3; ++ci) bias[ci] = a.b_in[(cb0 + ci) * 16 + r16];

  // ---- 1. GroupNorm statistics from the registers (two passes, fixed reduction order) -----------------
  const int grp = q4 >> 2;                                     // 4 quads per group, in adjacent lanes
  auto group_sum = [&](float v, float *slot) -> float {        // `slot`: 128 floats of its own (no barrier behind the reads)
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 32);                                    // the wave's two row lanes
    if ((lane & 35) == 0) slot[wave * 8 + grp] = v;
    __syncthreads();
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) t += slot[w * 8 + grp];  // every thread, the same order
    return t;
  };
  float s1 = 0.f;
#pragma unroll
  for (int u = 0; u < 2; ++u)
    if (rl + 32 * u < S) s1 += (vx[u][0] + vx[u][1]) + (vx[u][2] + vx[u][3]);
  const float cnt = (float)(E / 8) * (float)S;
  const float mean = group_sum(s1, red) / cnt;
  float s2 = 0.f;
#pragma unroll
  for (int u = 0; u < 2; ++u)
    if (rl + 32 * u < S) {
      const float d0 = vx[u][0] - mean, d1 = vx[u][1] - mean, d2 = vx[u][2] - mean, d3 = vx[u][3] - mean;
      s2 += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
    }
  const float rstd = rsqrtf(group_sum(s2, red + 128) / cnt + a.eps);      // biased variance (nn.GroupNorm)

  // ---- 2. xn, its range, the (hi, mid) planes -----------------------------------------------------------
  f32x4 xn[2];
  float amax = 0.f;
  {
    const f32x4 sc = ga * rstd;
    const f32x4 sh = be - sc * mean;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      xn[u] = vx[u] * sc + sh;
      if (rl + 32 * u < S) amax = fmaxf(amax, fmaxf(fmaxf(fabsf(xn[u][0]), fabsf(xn[u][1])), fmaxf(fabsf(xn[u][2]), fabsf(xn[u][3]))));
      else xn[u] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }
  auto sample_max = [&](float v, float *slot) -> float {       // max over the workgroup; `slot`: 16 floats nobody else uses
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    if (lane == 0) slot[wave] = v;
    __syncthreads();
    float m = slot[0];
#pragma unroll
    for (int w = 1; w < NT / 64; ++w) m = fmaxf(m, slot[w]);
    return m;
  };
  float isa;
  const float sa = as_range_scale(sample_max(amax, red + 272), &isa);
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    cm_u32x2_t t3[3];
    cm_split2_f16(xn[u] * sa, t3);
    const int row = rl + 32 * u;
    *reinterpret_cast<cm_u32x2_t *>(XH + row * HS + 4 * q4) = t3[0];
    *reinterpret_cast<cm_u32x2_t *>(XM + row * HS + 4 * q4) = t3[1];
  }
  __syncthreads();

  // ---- 3. in-projection -------------------------------------------------------------------------------
  {
    const float osc = a.in_oscale * isa, qscale = rsqrtf((float)D);
#pragma unroll
    for (int ci = 0; ci < 3; ++ci) {
      const int cb = cb0 + ci;
      const int which = cb >> 3, c = (cb & 7) * 16 + r16;      // q | k | v, column inside it
      float *dst = which == 0 ? Qs : (which == 1 ? Ks : Vs);
      for (int rb = rbp; rb < nrb; rb += 2) {
        const _Float16 *ah = XH + (rb * 16 + r16) * HS + 8 * g4, *am = XM + (rb * 16 + r16) * HS + 8 * g4;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          const f16x8a xh = *reinterpret_cast<const f16x8a *>(ah + 32 * ks), xm = *reinterpret_cast<const f16x8a *>(am + 32 * ks);
          const f16x8a wh = __builtin_bit_cast(f16x8a, wf[ci][ks][0]), wm = __builtin_bit_cast(f16x8a, wf[ci][ks][1]);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(xh, wm, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(xm, wh, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(xh, wh, acc, 0, 0, 0);
        }
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          float v = acc[reg] * osc + bias[ci];
          if (which == 0) v *= qscale;
          dst[(rb * 16 + 4 * g4 + reg) * QS + c] = v;          // rows >= S of a block: the bias, never read as a token
        }
      }
      if (ci == 0) {                                           // the third column block, into the first one's registers' worth: in flight across the second
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
#pragma unroll
          for (int t = 0; t < 2; ++t) wf[2][ks][t] = wing[(((size_t)(cb0 + 2) * 4 + ks) * 2 + t) * 64 + lane];
      }
    }
  }
  // the out-projection fragments of this wave (column block wave / 2): in flight across the attention phase
  const u32x4a *woutg = reinterpret_cast<const u32x4a *>(a.wout_h2);
  const f32x4 bo = *reinterpret_cast<const f32x4 *>(a.b_out + 4 * q4);
#pragma unroll
  for (int u = 0; u < 2; ++u)                                  // the residual again (the registers were the in-projection's): same addresses
    vx[u] = *reinterpret_cast<const f32x4 *>(xb + (size_t)min(rl + 32 * u, S - 1) * E + 4 * q4);
#pragma unroll
  for (int ks = 0; ks < 4; ++ks)
#pragma unroll
    for (int t = 0; t < 2; ++t) wf[0][ks][t] = woutg[(((size_t)(wave >> 1) * 4 + ks) * 2 + t) * 64 + lane];
  __syncthreads();

  // ---- 4. attention: wave = (head, 16 queries) ----------------------------------------------------------
  const int h = wave >> 2, qb = wave & 3;
  f32x4 oT[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};  // O^T: dims 16 db + 4 g4 + reg of query qb * 16 + r16
  float omax = 0.f;
  const bool qvalid = qb * 16 + r16 < S;
  if (qb < nrb) {
    const float *qp = Qs + (qb * 16 + r16) * QS + h * D + 8 * g4;
    const f32x4 q0 = *reinterpret_cast<const f32x4 *>(qp), q1 = *reinterpret_cast<const f32x4 *>(qp + 4);
    f32x4 sc[4];
    float mx = -3.0e38f;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
      sc[kb] = f32x4{-3.0e38f, -3.0e38f, -3.0e38f, -3.0e38f};
      if (kb < nrb) {
        const float *kp = Ks + (kb * 16 + r16) * QS + h * D + 8 * g4;
        const f32x4 k0 = *reinterpret_cast<const f32x4 *>(kp), k1 = *reinterpret_cast<const f32x4 *>(kp + 4);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(k0[j], q0[j], acc, 0, 0, 0);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(k1[j], q1[j], acc, 0, 0, 0);
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {                    // key kb * 16 + 4 g4 + reg
          sc[kb][reg] = (kb * 16 + 4 * g4 + reg < S) ? acc[reg] : -3.0e38f;
          mx = fmaxf(mx, sc[kb][reg]);
        }
      }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    float l = 0.f;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const float p = (kb < nrb && kb * 16 + 4 * g4 + reg < S) ? __expf(sc[kb][reg] - mx) : 0.f;
        sc[kb][reg] = p;
        l += p;
      }
    l += __shfl_xor(l, 16);
    l += __shfl_xor(l, 32);
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
      if (kb < nrb) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const float *vp = Vs + (kb * 16 + 4 * g4 + reg) * QS + h * D + r16;
          oT[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(vp[0], sc[kb][reg], oT[0], 0, 0, 0);
          oT[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(vp[16], sc[kb][reg], oT[1], 0, 0, 0);
        }
      }
    const float inv = 1.0f / l;
    oT[0] *= inv;
    oT[1] *= inv;
    if (qvalid) {
#pragma unroll
      for (int db = 0; db < 2; ++db)
        omax = fmaxf(omax, fmaxf(fmaxf(fabsf(oT[db][0]), fabsf(oT[db][1])), fmaxf(fabsf(oT[db][2]), fabsf(oT[db][3]))));
    }
  }
  float iso;
  const float so = as_range_scale(sample_max(omax, red + 288), &iso);   // (its barrier: every wave is past the xn planes and q)
  if (qb < nrb) {
#pragma unroll
    for (int db = 0; db < 2; ++db) {
      cm_u32x2_t t3[3];
      cm_split2_f16(qvalid ? oT[db] * so : f32x4{0.f, 0.f, 0.f, 0.f}, t3);
      const int off = (qb * 16 + r16) * HS + h * D + 16 * db + 4 * g4;
      *reinterpret_cast<cm_u32x2_t *>(XH + off) = t3[0];
      *reinterpret_cast<cm_u32x2_t *>(XM + off) = t3[1];
    }
  }
  __syncthreads();

  // ---- 5. out-projection: column block wave / 2, row blocks rbp, rbp + 2; y over q ---------------------------
  {
    const float osc = a.out_oscale * iso;
    const int c = (wave >> 1) * 16 + r16;
    for (int rb = rbp; rb < nrb; rb += 2) {
      const _Float16 *ah = XH + (rb * 16 + r16) * HS + 8 * g4, *am = XM + (rb * 16 + r16) * HS + 8 * g4;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const f16x8a xh = *reinterpret_cast<const f16x8a *>(ah + 32 * ks), xm = *reinterpret_cast<const f16x8a *>(am + 32 * ks);
        const f16x8a wh = __builtin_bit_cast(f16x8a, wf[0][ks][0]), wm = __builtin_bit_cast(f16x8a, wf[0][ks][1]);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(xh, wm, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(xm, wh, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(xh, wh, acc, 0, 0, 0);
      }
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) Qs[(rb * 16 + 4 * g4 + reg) * QS + c] = acc[reg] * osc;
    }
  }
  __syncthreads();

  // ---- 6. + bias + residual, stores; slot statistics of the result ---------------------------------------
  float *ob = a.out + (size_t)b * S * E;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int row = rl + 32 * u;
    if (row < S) {
      f32x4 *yp = reinterpret_cast<f32x4 *>(Qs + row * QS + 4 * q4);
      const f32x4 y = (*yp + bo) + vx[u];
      *yp = y;
      *reinterpret_cast<f32x4 *>(ob + (size_t)row * E + 4 * q4) = y;
    }
  }
  if (!a.stat_part) return;
  __syncthreads();
  if (tid < E * a.nslots) {
    const int c = tid & (E - 1), slot = tid >> 7;
    const int r0 = slot * 32, r1 = min(S, r0 + 32);
    float tot = 0.f;
    for (int r = r0; r < r1; ++r) tot += Qs[r * QS + c];
    const float n = (float)(r1 - r0);
    const float mu = tot / n;
    float m2 = 0.f;
    for (int r = r0; r < r1; ++r) { const float d = Qs[r * QS + c] - mu; m2 += d * d; }
    float *sp = a.stat_part + (((size_t)b * a.nslots + slot) * E + c) * 2;
    sp[0] = mu;
    sp[1] = m2;
    if (c == 0) a.stat_cnt[(size_t)b * a.nslots + slot] = n;
  }
}

hipError_t launch_attn_sample(const AttnSampleArgs &a, hipStream_t st) {
  if (!attn_sample_ok(a.S, AS_E, 4, 8) || a.B < 1 || a.nslots != (a.S + 31) / 32 || !a.win_h2 || !a.wout_h2) return hipErrorInvalidValue;
  static std::atomic<bool> attr_set[64];                       // (two lanes' host threads may launch on one device: setting it twice is harmless)
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (!attr_set[dev & 63].load(std::memory_order_acquire)) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(attn_sample_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
    attr_set[dev & 63].store(true, std::memory_order_release);
  }
  hipLaunchKernelGGL(attn_sample_kernel, dim3(a.B), dim3(AS_NT), attn_sample_lds_bytes(), st, a);
  return hipGetLastError();
}

}  // namespace cm
