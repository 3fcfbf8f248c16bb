// f16-operand staging shared by dit_gemm_f16_kernel (cm_dit.hip) and ditt_gemm_f16_kernel (cm_dit_train.hip): the token GEMMs of a
// DDPM-DiT training step under autocast (cm_dit4d_train_set_autocast) and, dit_gemm_f16_kernel alone, of the eval forward of a handle
// on the f16 sampling plan (cm_model_set_precision(CM_PRECISION_F16)).  Device code only.
//
// Instruction: v_mfma_f32_32x32x16_f16.  Lane l supplies A[row l & 31][k = 8 (l >> 5) + j] and B[k = 8 (l >> 5) + j][col l & 31],
// j = 0..7, as one f16x8; the C/D map is the fp32 instruction's (column = l & 31, row = (i & 3) + 8 (i >> 2) + 4 (l >> 5)).
//
// Rounding: an operand is rounded once, fp32 -> f16 round-to-nearest-even (v_cvt_f16_f32; no clamp, so a value outside f16's
// range becomes +-inf and surfaces as a non-finite loss or gradient), when it is staged into LDS -- or, the weights of the f16
// sampling plan, by the same rule on the host when the handle is finalized (dit_finalize), and staged as they are.  Products are
// exact in the matrix unit and the accumulator, the partials and every output are fp32.
//
// The f16a plan of an FM-DiT handle (cm_model_set_precision(CM_PRECISION_F16A)) applies the same rule to its four token Linears and,
// in dit_attn_full_f16_kernel (cm_dit.hip), to both attention products: q * 0.125 is formed in fp32 and then rounded; k and v are
// rounded when loaded; p = expf(s - m) is fp32, the softmax denominator accumulates the UNROUNDED p, and p is rounded as the
// operand of p v; the rescale by exp(m_old - m_new) and the final o / den are fp32.
//
// LDS image of either operand: [64 tile rows or columns][DH_K = 64 k] halves, k contiguous, row stride DH_S = 72 halves = 144 B =
// 36 dwords.  Operand read: one 16-byte ds_read_b128 per lane and k step at row * 144 + 32 step + 16 (l >> 5).  That instruction
// is served in four 16-lane groups ({0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32), bank = (byte / 4) mod 64; the 16
// rows of a group are distinct mod 16 and 36 r mod 64 = 4 (9 r mod 16), so they fall on 16 distinct 16-byte slots: conflict-free.
// Staging writes are 16-byte ds_write_b128 (eight consecutive k of one row), served in groups of 8 consecutive lanes on
// (byte / 4) mod 32: the k-contiguous staging gives a group the 128 contiguous bytes of one row; the transposing staging of
// ditt_gemm_f16_kernel gives it 8 rows distinct mod 8 (see there), 36 r mod 32 = 4 (9 r mod 8): conflict-free as well.
#pragma once

#include <stdint.h>

namespace cm {

typedef _Float16 dit_f16x8 __attribute__((ext_vector_type(8)));

constexpr int DH_K = 64;         // k chunk staged in LDS
constexpr int DH_S = DH_K + 8;   // row stride in halves

// elements k .. k + 7 of the row at p, zero at and past K
__device__ __forceinline__ void dh_load8(const float *__restrict__ p, long long k, long long K, float v[8]) {
  if (k + 8 <= K && (((uintptr_t)(p + k)) & 15) == 0) {
    const float4 x = *(const float4 *)(p + k), y = *(const float4 *)(p + k + 4);
    v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w; v[4] = y.x; v[5] = y.y; v[6] = y.z; v[7] = y.w;
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = k + e < K ? p[k + e] : 0.f;
  }
}

__device__ __forceinline__ dit_f16x8 dh_round8(const float v[8]) {
  dit_f16x8 h;
#pragma unroll
  for (int e = 0; e < 8; ++e) h[e] = (_Float16)v[e];
  return h;
}

// one k chunk of a 32 x 32 wave tile: ap / bp point at the lane's row of each image, at k = 8 (l >> 5)
template <typename ACC>
__device__ __forceinline__ ACC dh_mfma_chunk(const _Float16 *ap, const _Float16 *bp, ACC acc) {
#pragma unroll
  for (int s = 0; s < DH_K / 16; ++s)
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(*(const dit_f16x8 *)(ap + 16 * s), *(const dit_f16x8 *)(bp + 16 * s), acc, 0, 0, 0);
  return acc;
}

}  // namespace cm
