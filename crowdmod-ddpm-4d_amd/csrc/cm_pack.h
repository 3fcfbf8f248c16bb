// Weight-fragment layouts of the UNet's conv and attention kernels: host only, no HIP calls, no model types.
//
// Every layout is written down ONCE, as a function template over the element type.  On float it gives the fragments a handle
// uploads when it loads (cm_model.cpp: add_conv); on int (pad -1), fed with the positions of the reference weight in the flat
// parameter buffer, it gives the map the device re-packs through after an optimizer step (cm_train_host.inc: train_setup).  The
// parity-mode upsample conv, whose packed element is a sum of up to 8 reference weights, maps through Src8 elements.  The f16 and
// split (bf16 x 3, h2) flavours are conversions of a layout's fp32 fragments or share one walk.
#pragma once

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace cm_pack {

// ---- number formats ------------------------------------------------------------------------------------------------------------
// IEEE binary16 bits of a float (round to nearest even; overflow -> infinity, like a device cast)
inline uint16_t f32_to_f16_bits(float f) {
  uint32_t x;
  std::memcpy(&x, &f, 4);
  const uint32_t sign = (x >> 16) & 0x8000u;
  const int32_t exp = (int32_t)((x >> 23) & 0xff) - 127 + 15;
  uint32_t man = x & 0x7fffffu;
  if (((x >> 23) & 0xff) == 0xff) return (uint16_t)(sign | 0x7c00u | (man ? 0x200u : 0));
  if (exp >= 31) return (uint16_t)(sign | 0x7c00u);
  if (exp <= 0) {
    if (exp < -10) return (uint16_t)sign;
    man |= 0x800000u;
    const int shift = 14 - exp;
    uint32_t h = man >> shift;
    const uint32_t rem = man & ((1u << shift) - 1), half = 1u << (shift - 1);
    if (rem > half || (rem == half && (h & 1))) ++h;
    return (uint16_t)(sign | h);
  }
  uint32_t h = ((uint32_t)exp << 10) | (man >> 13);
  const uint32_t rem = man & 0x1fffu;
  if (rem > 0x1000u || (rem == 0x1000u && (h & 1))) ++h;
  return (uint16_t)(sign | h);
}
// IEEE binary16 bits -> float (exact)
inline float f16_bits_to_f32(uint16_t h) {
  const uint32_t sign = (uint32_t)(h & 0x8000u) << 16;
  uint32_t exp = (h >> 10) & 0x1fu, man = h & 0x3ffu, x;
  if (exp == 0) {
    if (man == 0) { x = sign; }
    else {
      int e = -1;
      do { ++e; man <<= 1; } while (!(man & 0x400u));
      x = sign | ((uint32_t)(127 - 15 - e) << 23) | ((man & 0x3ffu) << 13);
    }
  } else if (exp == 31) {
    x = sign | 0x7f800000u | (man << 13);
  } else {
    x = sign | ((exp + 127 - 15) << 23) | (man << 13);
  }
  float f;
  std::memcpy(&f, &x, 4);
  return f;
}
// round-to-nearest-even fp32 -> bf16 (bits)
inline uint16_t f32_to_bf16_bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);   // NaN stays NaN
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
inline float bf16_bits_to_f32(uint16_t h) {
  const uint32_t u = (uint32_t)h << 16;
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}
// h2 terms of one weight (cm_kernels.h: cm_split2_f16): f16 hi / mid of w * scale, third slot zero
inline void f16_split2(float w, float scale, uint16_t out[3]) {
  const float v = w * scale;
  out[0] = f32_to_f16_bits(v);
  out[1] = f32_to_f16_bits(v - f16_bits_to_f32(out[0]));
  out[2] = 0;
}
// exact three-way bf16 split of an fp32 value: w = hi + mid + lo (each rounded to nearest from the running remainder;
// 8 + 8 + 8 mantissa bits, the remainders are exact in fp32)
inline void bf16_split3(float w, uint16_t out[3]) {
  float rem = w;
  for (int t = 0; t < 3; ++t) {
    out[t] = f32_to_bf16_bits(rem);
    rem -= bf16_bits_to_f32(out[t]);
  }
}
// the three 16-bit terms of one weight in a split fragment: h2 (f16 hi / mid of w * h2_scale) when h2_scale > 0, else bf16 x 3
inline void split_terms(float w, float h2_scale, uint16_t out[3]) {
  if (h2_scale > 0.f) f16_split2(w, h2_scale, out);
  else bf16_split3(w, out);
}
// 16-bit fragments are uploaded as floats holding two of them each
inline std::vector<float> halves_as_floats(const std::vector<uint16_t> &h) {
  std::vector<float> packed(h.size() / 2);
  std::memcpy(packed.data(), h.data(), packed.size() * 4);
  return packed;
}
// f16 flavour of an fp32 fragment vector: the same order, element by element (zero padding stays zero)
inline std::vector<float> fragments_f16(const std::vector<float> &f) {
  std::vector<uint16_t> h(f.size());
  for (size_t i = 0; i < f.size(); ++i) h[i] = f32_to_f16_bits(f[i]);
  return halves_as_floats(h);
}

// "h2" arithmetic (cm_kernels.h: cm_split2_f16), operand range management of the weights: f16 has 5 exponent bits, so a layer's
// weights are packed as w * 2^k with max |w| 2^k in [4096, 8192) (their mid terms ~ 2^-11 of that stay normal numbers; 8x headroom
// below 65504) and the kernel multiplies its fp32 accumulators by 2^-k (exact).  Returns 2^k; 0: none (all-zero or non-finite).
inline float h2_wscale(const float *w, size_t n) {
  float mx = 0.f;
  for (size_t i = 0; i < n; ++i) mx = std::max(mx, std::fabs(w[i]));
  if (!(mx > 0.f) || !std::isfinite(mx)) return 0.f;
  int e = 0;
  (void)std::frexp(mx, &e);                        // mx = f * 2^e, f in [0.5, 1)
  return std::ldexp(1.0f, 13 - e);                 // mx * 2^(13 - e) in [4096, 8192)
}

// ---- reference tap order -------------------------------------------------------------------------------------------------------
// Reference conv weight [Co][Ci][kH][kW][kL] -> internal tap order [Co][Ci][t], t = (dz*3 + dy)*3 + dx
// with (dz,dy,dx) = (kL,kH,kW)  (the internal layout is [Z=frames][Y=rows][X=cols]).  ntaps = 1: a copy.
template <class T>
std::vector<T> to_internal_taps(const T *W, int Co, int Ci, int ntaps) {
  std::vector<T> out((size_t)Co * Ci * ntaps);
  for (size_t cc = 0; cc < (size_t)Co * Ci; ++cc)
    for (int t = 0; t < ntaps; ++t) {
      const int dz = t / 9, dy = (t / 3) % 3, dx = t % 3;
      const int tap_ref = (ntaps == 27) ? (dy * 3 + dx) * 3 + dz : 0;
      out[cc * ntaps + t] = W[cc * ntaps + tap_ref];
    }
  return out;
}

// ---- generic MFMA fragment order (the kernels' comments call it the pack_conv_weights order) ----------------------------------
//   wfrag[ntile][chunk][step = tap*K8 + j][nb][lane][jj]
//     = src[co = ntile*TN + nb*32 + (lane&31)][ci = chunk*CK + 8j + 4(lane>>5) + jj][tap],   src: [Co][Ci][ntaps]
// `pad` beyond Co / Ci.  One wave-load of a step is 64 lanes x 16 B = 1 KiB contiguous.
template <class T>
std::vector<T> pack_conv(const T *src, int Co, int Ci, int ntaps, int Ci_pad, int CK, int NB, T pad = T{}) {
  const int TN = 32 * NB, ntn = (Co + TN - 1) / TN, nch = Ci_pad / CK, K8 = CK / 8, nsteps = ntaps * K8;
  std::vector<T> out((size_t)ntn * nch * nsteps * NB * 64 * 4, pad);
  size_t o = 0;
  for (int nt = 0; nt < ntn; ++nt)
    for (int ch = 0; ch < nch; ++ch)
      for (int s = 0; s < nsteps; ++s) {
        const int t = s / K8, j = s % K8;
        for (int nb = 0; nb < NB; ++nb)
          for (int lane = 0; lane < 64; ++lane)
            for (int jj = 0; jj < 4; ++jj, ++o) {
              const int co = nt * TN + nb * 32 + (lane & 31);
              const int ci = ch * CK + 8 * j + 4 * (lane >> 5) + jj;
              if (co < Co && ci < Ci) out[o] = src[((size_t)co * Ci + ci) * ntaps + t];
            }
      }
  return out;
}

// its f16 flavour (cm_conv.hip, F16 plan): the same order, 4 halves per lane and step
inline std::vector<float> pack_conv_f16(const float *src, int Co, int Ci, int ntaps, int Ci_pad, int CK, int NB) {
  return fragments_f16(pack_conv(src, Co, Ci, ntaps, Ci_pad, CK, NB));
}

// ---- parity form of the upsample conv ------------------------------------------------------------------------------------------
// nn.Upsample(x2, nearest) followed by a 3x3x3 conv (layers.py:93-94) collapses, for each
// parity p of the output voxel u = 2i + p, to a 2x2x2 conv over source voxels i + e + p - 1:
// along one axis tap d of the upsampled grid reads source floor((2i + p + d - 1)/2), i.e.
//   p = 0: d=0 -> i-1 (e=0), d=1,2 -> i (e=1);    p = 1: d=0,1 -> i (e=0), d=2 -> i+1 (e=1).
// The e slot (ez*2 + ey)*2 + ex that tap (dz, dy, dx) of parity class p = (pz*2 + py)*2 + px folds into:
inline int parity_slot(int p, int dz, int dy, int dx) {
  auto axis = [](int pa, int d) { return pa == 0 ? (d == 0 ? 0 : 1) : (d == 2 ? 1 : 0); };
  return (axis((p >> 2) & 1, dz) * 2 + axis((p >> 1) & 1, dy)) * 2 + axis(p & 1, dx);
}
// Taps that land on the same source voxel are summed (in double, in (dz, dy, dx) order, rounded once).
// in: internal order [Co][Ci][27]; out: [8 parities][Co][Ci][8 e slots].
inline std::vector<float> parity_weights(const std::vector<float> &Wi, int Co, int Ci) {
  std::vector<float> out((size_t)8 * Co * Ci * 8, 0.f);
  for (int p = 0; p < 8; ++p)
    for (size_t cc = 0; cc < (size_t)Co * Ci; ++cc) {
      double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      for (int dz = 0; dz < 3; ++dz)
        for (int dy = 0; dy < 3; ++dy)
          for (int dx = 0; dx < 3; ++dx) acc[parity_slot(p, dz, dy, dx)] += (double)Wi[cc * 27 + (dz * 3 + dy) * 3 + dx];
      for (int e = 0; e < 8; ++e) out[((size_t)p * Co * Ci + cc) * 8 + e] = (float)acc[e];
    }
  return out;
}
// The same fold on indices: per element of parity_weights' output, the (up to 8) sources it sums, in the same order, -1 beyond.
using Src8 = std::array<int, 8>;
constexpr Src8 kNoSrc8 = {-1, -1, -1, -1, -1, -1, -1, -1};
inline std::vector<Src8> parity_sources(const std::vector<int> &ii, int Co, int Ci) {
  std::vector<Src8> out((size_t)8 * Co * Ci * 8, kNoSrc8);
  for (int p = 0; p < 8; ++p)
    for (size_t cc = 0; cc < (size_t)Co * Ci; ++cc) {
      int fill[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      for (int dz = 0; dz < 3; ++dz)
        for (int dy = 0; dy < 3; ++dy)
          for (int dx = 0; dx < 3; ++dx) {
            const int e = parity_slot(p, dz, dy, dx);
            out[((size_t)p * Co * Ci + cc) * 8 + e][fill[e]++] = ii[cc * 27 + (dz * 3 + dy) * 3 + dx];
          }
    }
  return out;
}
// A per-class packer applied to the 8 parity classes of `wp` ([8][Co][Ci][8]), concatenated; *stride = elements per class.
template <class T, class PackOne>
auto pack_parity_classes(const std::vector<T> &wp, long long *stride, PackOne pack_one) -> decltype(pack_one(wp.data())) {
  decltype(pack_one(wp.data())) all;
  const size_t per = wp.size() / 8;
  for (int p8 = 0; p8 < 8; ++p8) {
    const auto one = pack_one(wp.data() + p8 * per);
    *stride = (long long)one.size();
    all.insert(all.end(), one.begin(), one.end());
  }
  return all;
}

// 16-bit fragments of ONE parity class for the stage-once upsample kernel (cm_conv_ups.hip): [32-channel column block]
// [32-channel chunk][tap 8][16-channel group m][term NT][lane][8], lane = 32 hh + (co % 32), ci = chunk * 32 + 16 m + 8 hh + i.
// W: [Co][Ci][8] (parity_weights of one class); terms(w, t) writes the NT 16-bit terms of one weight.
template <int NT, class Terms>
std::vector<float> pack_ups_terms(const float *W, int Co, int Ci, Terms terms) {
  const int ncb = Co / 32, nch = Ci / 32;
  std::vector<uint16_t> out((size_t)ncb * nch * 8 * 2 * NT * 64 * 8, 0);
  for (int cb = 0; cb < ncb; ++cb)
    for (int ch = 0; ch < nch; ++ch)
      for (int t = 0; t < 8; ++t)
        for (int mg = 0; mg < 2; ++mg)
          for (int lane = 0; lane < 64; ++lane)
            for (int i = 0; i < 8; ++i) {
              const int co = cb * 32 + (lane & 31), ci = ch * 32 + 16 * mg + 8 * (lane >> 5) + i;
              uint16_t t3[3];
              terms(W[((size_t)co * Ci + ci) * 8 + t], t3);
              for (int tm = 0; tm < NT; ++tm)
                out[(((((((size_t)cb * nch + ch) * 8 + t) * 2 + mg) * NT + tm) * 64) + lane) * 8 + i] = t3[tm];
            }
  return halves_as_floats(out);
}
// F16 form: one f16 term
inline std::vector<float> pack_ups_f16(const float *W, int Co, int Ci) {
  return pack_ups_terms<1>(W, Co, Ci, [](float w, uint16_t *t3) { t3[0] = f32_to_f16_bits(w); });
}
// PREC = 2: bf16 hi / mid / lo; h2_scale > 0: the h2 form -- f16 hi / mid of w * h2_scale in the first two term slots (third slot zero)
inline std::vector<float> pack_ups_b6(const float *W, int Co, int Ci, float h2_scale = 0.f) {
  return pack_ups_terms<3>(W, Co, Ci, [h2_scale](float w, uint16_t *t3) { split_terms(w, h2_scale, t3); });
}

// ---- Winograd layers -----------------------------------------------------------------------------------------------------------
// Winograd F(2x2, 3x3) weights over the in-plane taps (dy, dx), one 4x4 transform G g G^T per (co, ci, dz):
//   G = (1,0,0), (1/2,1/2,1/2), (1/2,-1/2,1/2), (0,0,1).
// Element (xi_y, xi_x) of it, in double; `wi` is the internal tap order [Co][Ci][27].
inline double wino_tap(const std::vector<float> &wi, int Ci, int co, int ci, int dz, int xy, int xx) {
  static const double G[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
  double acc = 0;
  for (int dy = 0; dy < 3; ++dy)
    for (int dx = 0; dx < 3; ++dx) acc += G[xy][dy] * G[xx][dx] * (double)wi[((size_t)co * Ci + ci) * 27 + (dz * 3 + dy) * 3 + dx];
  return acc;
}
// fp32 layout (cm_conv_wino.hip): [n tile][16-channel chunk][xi_y][step = (dz*2 + k8)*4 + xi_x][lane][jj] with
// lane = 32*hh + (co % 32), ci = chunk*16 + 8*k8 + 4*hh + jj.
// (After an optimizer step the device re-derives it from the master weights: wino_pack_jobs_kernel.)
inline std::vector<float> pack_wino(const std::vector<float> &wi, int Co, int Ci, int Ci_pad) {
  const int ntn = (Co + 31) / 32, nch = Ci_pad / 16;
  std::vector<float> out((size_t)ntn * nch * 4 * 24 * 64 * 4, 0.f);
  for (int co = 0; co < Co; ++co)
    for (int ci = 0; ci < Ci; ++ci)
      for (int dz = 0; dz < 3; ++dz)
        for (int xy = 0; xy < 4; ++xy)
          for (int xx = 0; xx < 4; ++xx) {
            const int nt = co / 32, r = co % 32, chunk = ci / 16, k8 = (ci % 16) / 8, hh = (ci % 8) / 4, jj = ci % 4;
            const size_t o = ((((((size_t)nt * nch + chunk) * 4 + xy) * 24 + (dz * 2 + k8) * 4 + xx) * 64) + hh * 32 + r) * 4 + jj;
            out[o] = (float)wino_tap(wi, Ci, co, ci, dz, xy, xx);
          }
  return out;
}
// f16 packing of the Winograd weights (cm_conv_wino.hip, F16): [n tile][chunk][xi_y][dz][xi_x][lane][8 halves],
// lane = 32*hh + co % 32, ci = chunk*16 + 8*hh + j.
inline std::vector<float> pack_wino_f16(const std::vector<float> &wi, int Co, int Ci, int Ci_pad) {
  const int ntn = (Co + 31) / 32, nch = Ci_pad / 16;
  std::vector<uint16_t> out((size_t)ntn * nch * 4 * 3 * 4 * 64 * 8, 0);
  for (int co = 0; co < Co; ++co)
    for (int ci = 0; ci < Ci; ++ci)
      for (int dz = 0; dz < 3; ++dz)
        for (int xy = 0; xy < 4; ++xy)
          for (int xx = 0; xx < 4; ++xx) {
            const int nt = co / 32, r = co % 32, chunk = ci / 16, hh = (ci % 16) / 8, j = ci % 8;
            const size_t o = (((((((size_t)nt * nch + chunk) * 4 + xy) * 3 + dz) * 4 + xx) * 64) + hh * 32 + r) * 8 + j;
            out[o] = f32_to_f16_bits((float)wino_tap(wi, Ci, co, ci, dz, xy, xx));
          }
  return halves_as_floats(out);
}
// Six-term bf16 form of the Winograd layers (conv_wino_p_kernel<..., B6>): the fp32 fragments of pack_wino
// ([n tile][chunk][xi_y][step = (dz * 2 + k8) * 4 + xi_x][lane][4], ci = chunk * 16 + 8 k8 + 4 hh + jj) split exactly into three
// bf16 terms and regrouped as [n tile][chunk][xi_y][dz][xi_x][term][lane][8 bf16], ci = chunk * 16 + 8 hh + j.  The device
// re-derives the same thing after an optimizer step (wino_b6_repack_kernel): one definition, two places -- the self-test
// compares them element by element.
// h2_scale > 0: the h2 form instead -- f16 hi / mid of w * h2_scale in the first two term slots (same layout, third slot zero)
inline std::vector<float> pack_wino_b6(const std::vector<float> &ww, float h2_scale = 0.f) {
  std::vector<uint16_t> out(ww.size() * 3, 0);
  for (size_t i = 0; i < ww.size(); ++i) {
    const int jj = (int)(i & 3), lane = (int)((i >> 2) & 63);
    size_t q = i >> 8;
    const int step = (int)(q % 24); q /= 24;
    const int xy = (int)(q & 3);
    const size_t tc = q >> 2;
    const int xx = step & 3, k8 = (step >> 2) & 1, dz = step >> 3;
    const int r = lane & 31, hs = lane >> 5, cl = 8 * k8 + 4 * hs + jj, hd = cl >> 3, j = cl & 7;
    uint16_t t3[3];
    split_terms(ww[i], h2_scale, t3);
    for (int tm = 0; tm < 3; ++tm)
      out[(((((((tc * 4 + xy) * 3 + dz) * 4 + xx) * 3 + tm) * 64) + 32 * hd + r) * 8) + j] = t3[tm];
  }
  return halves_as_floats(out);
}

// ---- f16 plan ------------------------------------------------------------------------------------------------------------------
// f16 fragments of a 1x1x1 conv for conv1x1_f16_kernel: [n tile][16-channel group][block][lane 64][8 halves],
// lane (r, h) of block nb holds W[co = (nt NB + nb) 32 + r][ci = 16 g + 8 h + j]; W is [Co][Ci]
inline std::vector<float> pack_1x1_f16(const float *W, int Co, int Ci, int NB) {
  const int TN = 32 * NB, ntn = (Co + TN - 1) / TN, ng = Ci / 16;
  std::vector<uint16_t> out((size_t)ntn * ng * NB * 64 * 8, 0);
  size_t o = 0;
  for (int nt = 0; nt < ntn; ++nt)
    for (int g = 0; g < ng; ++g)
      for (int nb = 0; nb < NB; ++nb)
        for (int lane = 0; lane < 64; ++lane)
          for (int j = 0; j < 8; ++j, ++o) {
            const int co = (nt * NB + nb) * 32 + (lane & 31), ci = 16 * g + 8 * (lane >> 5) + j;
            if (co < Co) out[o] = f32_to_f16_bits(W[(size_t)co * Ci + ci]);
          }
  return halves_as_floats(out);
}
// f16 fragments of the direct f16 kernel (cm_conv_f16.hip): [Co/(32 NB)][Ci/16][taps][NB][lane][8 halves] with
// co = 32 NB nt + 32 nb + lane % 32, ci = 16 c + 8 (lane / 32) + j; `w` is [Co][Ci][taps] (taps = 27 internal order, or 1)
inline std::vector<float> pack_f16d(const float *w, int Co, int Ci, int taps, int NB) {
  const int ntn = Co / (32 * NB), nc = Ci / 16;
  std::vector<uint16_t> out((size_t)ntn * nc * taps * NB * 64 * 8, 0);
  size_t o = 0;
  for (int nt = 0; nt < ntn; ++nt)
    for (int c = 0; c < nc; ++c)
      for (int t = 0; t < taps; ++t)
        for (int nb = 0; nb < NB; ++nb)
          for (int lane = 0; lane < 64; ++lane)
            for (int j = 0; j < 8; ++j, ++o) {
              const int co = nt * 32 * NB + nb * 32 + (lane & 31), ci = 16 * c + 8 * (lane >> 5) + j;
              out[o] = f32_to_f16_bits(w[((size_t)co * Ci + ci) * taps + t]);
            }
  return halves_as_floats(out);
}

// ---- whole-sample quarter-resolution kernel (cm_conv_qr.hip) -------------------------------------------------------------------
// [Co/32][g = k8*9 + dy*3 + dx][dz][lane][jj] with co = 32 nt + lane % 32, ci = 8 k8 + 4 (lane / 32) + jj; `wi` in the internal
// tap order [Co][Ci][(dz*3 + dy)*3 + dx].  (The data gradient packs W'[ci][co][flipped tap] through it with Co and Ci swapped.)
template <class T>
std::vector<T> pack_qr(const std::vector<T> &wi, int Co, int Ci) {
  const int ntn = Co / 32, K8 = Ci / 8, ng = 9 * K8;
  std::vector<T> out((size_t)ntn * ng * 3 * 64 * 4);
  size_t o = 0;
  for (int nt = 0; nt < ntn; ++nt)
    for (int g = 0; g < ng; ++g)
      for (int dz = 0; dz < 3; ++dz)
        for (int lane = 0; lane < 64; ++lane)
          for (int jj = 0; jj < 4; ++jj, ++o) {
            const int k8 = g / 9, t9 = g % 9, dy = t9 / 3, dx = t9 % 3;
            const int co = nt * 32 + (lane & 31), ci = 8 * k8 + 4 * (lane >> 5) + jj;
            out[o] = wi[((size_t)co * Ci + ci) * 27 + (dz * 3 + dy) * 3 + dx];
          }
  return out;
}
// Six-term bf16 form of conv_qr2 (B6): the fp32 fragments of pack_qr split exactly into three bf16 terms and regrouped by wave
// (wave w owns the channels [w Ci/8, (w+1) Ci/8), padded with zeros to whole 16-channel steps):
// [Co/32][wave 8][step][tap 9][dz][term][lane][8 bf16], ci = wave * Ci/8 + 16 step + 8 hh + j.  `wq` is pack_qr's output.
// The device re-derives it after an optimizer step with the same index arithmetic (qr_b6_repack_kernel).
// h2_scale > 0: the h2 form (f16 hi / mid of w * h2_scale, third slot zero)
inline std::vector<float> pack_qr_b6(const std::vector<float> &wq, int Co, int Ci, float h2_scale = 0.f) {
  const int ntn = Co / 32, K8 = Ci / 8, ng = 9 * K8, cw = Ci / 8, nsw = (cw + 15) / 16;
  std::vector<uint16_t> out((size_t)ntn * 8 * nsw * 9 * 3 * 3 * 64 * 8, 0);
  for (size_t i = 0; i < wq.size(); ++i) {
    const int jj = (int)(i & 3), lane = (int)((i >> 2) & 63);
    size_t q = i >> 8;
    const int dz = (int)(q % 3); q /= 3;
    const int g = (int)(q % ng);
    const int nt = (int)(q / ng);
    const int k8 = g / 9, t9 = g % 9, ci = 8 * k8 + 4 * (lane >> 5) + jj, r = lane & 31;
    const int wv = ci / cw, cl = ci % cw, st = cl / 16, hd = (cl % 16) / 8, j = cl % 8;
    uint16_t t3[3];
    split_terms(wq[i], h2_scale, t3);
    for (int tm = 0; tm < 3; ++tm)
      out[(((((((size_t)(nt * 8 + wv) * nsw + st) * 9 + t9) * 3 + dz) * 3 + tm) * 64) + 32 * hd + r) * 8 + j] = t3[tm];
  }
  return halves_as_floats(out);
}
// its fused 1x1x1 skip weights: [Co/32][Cs/8][lane][jj]; `w2` is [Co][Cs]
template <class T>
std::vector<T> pack_qr_skip(const T *w2, int Co, int Cs) {
  const int ntn = Co / 32, ngs = Cs / 8;
  std::vector<T> out((size_t)ntn * ngs * 64 * 4);
  size_t o = 0;
  for (int nt = 0; nt < ntn; ++nt)
    for (int gs = 0; gs < ngs; ++gs)
      for (int lane = 0; lane < 64; ++lane)
        for (int jj = 0; jj < 4; ++jj, ++o)
          out[o] = w2[(size_t)(nt * 32 + (lane & 31)) * Cs + 8 * gs + 4 * (lane >> 5) + jj];
  return out;
}

// ---- the UNet's first and last conv --------------------------------------------------------------------------------------------
// First conv (Ci <= 8 data channels -> Co, cm_conv_io.hip: the whole weight set in registers): [Co/32][step = t * cin/2 + pp][lane]
// with co = 32 nt + lane % 32, ci = (cin/2) (lane / 32) + pp -- MFMA (t, pp) contracts k = {hc*hh + pp}; cin = 4 or 8 padded input
// channels, `pad` beyond Ci.  `wi`: [Co][Ci][27] internal order.
template <class T>
std::vector<T> pack_first(const T *wi, int Co, int Ci, int cin, T pad = T{}) {
  const int NS = 27 * cin / 2, hc = cin / 2, ntn = Co / 32;
  std::vector<T> out((size_t)ntn * NS * 64, pad);
  for (int nt = 0; nt < ntn; ++nt)
    for (int t = 0; t < 27; ++t)
      for (int pp = 0; pp < hc; ++pp)
        for (int lane = 0; lane < 64; ++lane) {
          const int co = nt * 32 + (lane & 31), ci = hc * (lane >> 5) + pp;
          if (ci < Ci) out[((size_t)nt * NS + t * hc + pp) * 64 + lane] = wi[((size_t)co * Ci + ci) * 27 + t];
        }
  return out;
}
// Last conv (Co <= 8 output channels, vector-ALU kernel cm_conv_small.hip): [chunk][tap 27][ci in chunk CK][nco] with nco = 4 or 8
// padded output channels, `pad` beyond Co / Ci.  `wi`: [Co][Ci][27] internal order.
template <class T>
std::vector<T> pack_small(const T *wi, int Co, int Ci, int Ci_pad, int CK, int nco, T pad = T{}) {
  const int nch = Ci_pad / CK;
  std::vector<T> out((size_t)nch * 27 * CK * nco, pad);
  for (int ch = 0; ch < nch; ++ch)
    for (int t = 0; t < 27; ++t)
      for (int ci = 0; ci < CK; ++ci)
        for (int co = 0; co < Co; ++co) {
          const int cig = ch * CK + ci;
          if (cig < Ci) out[(((size_t)ch * 27 + t) * CK + ci) * nco + co] = wi[((size_t)co * Ci + cig) * 27 + t];
        }
  return out;
}

// ---- whole-sample attention kernel ---------------------------------------------------------------------------------------------
// h2 fragments of a dense weight W [N][K] (reference layout: mhsa.in_proj_weight, mhsa.out_proj.weight) for the whole-sample
// attention kernel (cm_attn_block.hip: attn_sample_kernel): [16-column block][32-deep k step][hi, mid][lane][8 halves],
// lane = 16 g + (n % 16), k = 32 step + 8 g + i; f16 hi / mid of w * scale.
inline std::vector<float> pack_attn_h2(const float *W, int N, int K, float scale) {
  const int ncb = N / 16, nks = K / 32;
  std::vector<uint16_t> out((size_t)ncb * nks * 2 * 64 * 8, 0);
  for (int cb = 0; cb < ncb; ++cb)
    for (int ks = 0; ks < nks; ++ks)
      for (int lane = 0; lane < 64; ++lane)
        for (int i = 0; i < 8; ++i) {
          const int n = cb * 16 + (lane & 15), k = ks * 32 + 8 * (lane >> 4) + i;
          uint16_t t3[3];
          f16_split2(W[(size_t)n * K + k], scale, t3);
          for (int tm = 0; tm < 2; ++tm) out[(((((size_t)cb * nks + ks) * 2 + tm) * 64) + lane) * 8 + i] = t3[tm];
        }
  return halves_as_floats(out);
}

// ---- h2 fragments of a conv layer -----------------------------------------------------------------------------------------------
// From the layer's weight in the REFERENCE layout [Co][Ci][kH][kW][kL] (load time: add_conv; after training: refresh_h2): the scale
// 2^k is taken over the values the kernel multiplies (the fp32 fragments of its layout), then the split form of that layout is packed
// with it.  Returns 2^k; 0: none (all-zero or non-finite weights), *frag untouched.  H2_FIN (the last conv, cm_conv_fin.hip) only
// takes the scale here: its fragments are packed on the device (launch_fin_pack).
enum H2Kind { H2_FIN, H2_WINO, H2_QR, H2_UPS };
inline float h2_fragments(H2Kind kind, const float *w_ref, int Co, int Ci, std::vector<float> *frag) {
  if (kind == H2_FIN) return h2_wscale(w_ref, (size_t)Co * Ci * 27);
  const std::vector<float> wi = to_internal_taps(w_ref, Co, Ci, 27);
  const std::vector<float> f32 = kind == H2_WINO ? pack_wino(wi, Co, Ci, Ci) : kind == H2_QR ? pack_qr(wi, Co, Ci) : parity_weights(wi, Co, Ci);
  const float ws = h2_wscale(f32.data(), f32.size());
  if (!(ws > 0.f)) return ws;
  long long stride = 0;
  if (kind == H2_WINO) *frag = pack_wino_b6(f32, ws);
  else if (kind == H2_QR) *frag = pack_qr_b6(f32, Co, Ci, ws);
  else *frag = pack_parity_classes(f32, &stride, [&](const float *cls) { return pack_ups_b6(cls, Co, Ci, ws); });
  return ws;
}

}  // namespace cm_pack
