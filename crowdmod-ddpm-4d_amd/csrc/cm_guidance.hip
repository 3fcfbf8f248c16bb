// mass_preservation guidance (models/guidance.py:44-69, applied at ddpm.py:227-229):
//     g_i = (E(x + eps e_i) - E(x)) / eps,   x -= (1 - alpha_t) * g
// with E = 0.5 / (H W L) * sum_k f_k^2 the mass-conservation residual of compute_energy (guidance.py:10-42), cells
// k = (h, w, l), h in [1, H-2], w in [1, W-2], l in [0, L-2]:
//     f = (r[l+1] - r) / dt + r ((u[h+1] - u) + (v[w+1] - v)) / dl + (r[h+1] - r) u / dl + (r[w+1] - r) v / dl
// (r, u, v = channels 0, 1, 2).  No cell holds a product of one element with itself, so f_k is linear in every single
// element and the reference's forward-difference quotient is exactly
//     q_i = 0.5 / (H W L) * sum_{cells k touching i} g_ki (2 f_k + eps g_ki),   g_ki = df_k / dx_i
// -- at most four cells per element instead of one full energy evaluation per element.
#include <algorithm>

#include "cm_kernels.h"

namespace cm {

// Tile of one workgroup: th x tw x tl elements of one sample.  Staged in LDS: channels 0-2 over the tile plus a halo of
// one on each side in every dimension ((th+2)(tw+2)(tl+2) per channel), and the f cells that touch the tile (cells
// h0-1 .. h1-1 etc.: (th+1)(tw+1)(tl+1)).  Out-of-grid positions hold 0 and are never read by a valid cell.
static inline long long mass_tile_floats(int th, int tw, int tl) {
  return 3LL * (th + 2) * (tw + 2) * (tl + 2) + (long long)(th + 1) * (tw + 1) * (tl + 1);
}
static constexpr long long kMassLdsFloats = 8192;   // 32 KiB: five workgroups per CU

struct MassGradArgs {
  const float *x; int Cin;     // [B][Cin][H][W][L]
  float *q; int Cout;          // [B][Cout][H][W][L]: channels 0-2 = q, channels 3.. = 0
  int H, W, L;
  int th, tw, tl, nth, ntw, ntl;
  float inv_dt, inv_dl, eps, coef;   // coef = 0.5 / (H W L)
};

__global__ __launch_bounds__(256) void mass_grad_kernel(MassGradArgs a) {
  extern __shared__ float lds[];
  const int ntiles = a.nth * a.ntw * a.ntl;
  const int b = blockIdx.x / ntiles;
  int tix = blockIdx.x - b * ntiles;
  const int tl_i = tix % a.ntl; tix /= a.ntl;
  const int tw_i = tix % a.ntw;
  const int th_i = tix / a.ntw;
  const int h0 = th_i * a.th, w0 = tw_i * a.tw, l0 = tl_i * a.tl;
  const int H = a.H, W = a.W, L = a.L;
  const int SH = a.th + 2, SW = a.tw + 2, SL = a.tl + 2;    // staged x: origin (h0-1, w0-1, l0-1)
  const int FH = a.th + 1, FW = a.tw + 1, FL = a.tl + 1;    // f cells:  origin (h0-1, w0-1, l0-1)
  const int plane = SH * SW * SL;
  float *xs = lds;
  float *fs = lds + 3 * plane;
  const size_t HWL = (size_t)H * W * L;
  const float *xb = a.x + (size_t)b * a.Cin * HWL;

  // four independent loads in flight per thread before their LDS stores (one at a time leaves each load's latency exposed)
  for (int i0 = threadIdx.x; i0 < 3 * plane; i0 += 4 * 256) {
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int i = i0 + j * 256;
      v[j] = 0.f;
      if (i < 3 * plane) {
        const int c = i / plane;
        int e = i - c * plane;
        const int ll = e % SL; e /= SL;
        const int ww = e % SW;
        const int hh = e / SW;
        const int h = h0 - 1 + hh, w = w0 - 1 + ww, l = l0 - 1 + ll;
        if (h >= 0 && h < H && w >= 0 && w < W && l >= 0 && l < L) v[j] = xb[c * HWL + ((size_t)h * W + w) * L + l];
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (i0 + j * 256 < 3 * plane) xs[i0 + j * 256] = v[j];
  }
  __syncthreads();
  // x at grid position (h, w, l) of channel c (inside the staged box)
#define XS(c, h, w, l) xs[(c) * plane + (((h) - (h0 - 1)) * SW + ((w) - (w0 - 1))) * SL + ((l) - (l0 - 1))]
  for (int i = threadIdx.x; i < FH * FW * FL; i += 256) {
    int e = i;
    const int ll = e % FL; e /= FL;
    const int ww = e % FW;
    const int hh = e / FW;
    const int h = h0 - 1 + hh, w = w0 - 1 + ww, l = l0 - 1 + ll;
    float f = 0.f;
    if (h >= 1 && h <= H - 2 && w >= 1 && w <= W - 2 && l >= 0 && l <= L - 2) {
      const float r = XS(0, h, w, l), u = XS(1, h, w, l), v = XS(2, h, w, l);
      const float t1 = a.inv_dt * (XS(0, h, w, l + 1) - r);
      const float t2 = a.inv_dl * r * ((XS(1, h + 1, w, l) - u) + (XS(2, h, w + 1, l) - v));
      const float t3 = a.inv_dl * (XS(0, h + 1, w, l) - r) * u;
      const float t4 = a.inv_dl * (XS(0, h, w + 1, l) - r) * v;
      f = t1 + t2 + t3 + t4;
    }
    fs[i] = f;
  }
  __syncthreads();
#define FS(h, w, l) fs[(((h) - (h0 - 1)) * FW + ((w) - (w0 - 1))) * FL + ((l) - (l0 - 1))]
  auto cell = [&](int h, int w, int l) { return h >= 1 && h <= H - 2 && w >= 1 && w <= W - 2 && l >= 0 && l <= L - 2; };
  const int nel = a.th * a.tw * a.tl;
  float *qb = a.q + (size_t)b * a.Cout * HWL;
  for (int i = threadIdx.x; i < nel; i += 256) {
    int e = i;
    const int l = l0 + e % a.tl; e /= a.tl;
    const int w = w0 + e % a.tw;
    const int h = h0 + e / a.tw;
    if (h >= H || w >= W || l >= L) continue;
    const float r = XS(0, h, w, l), u = XS(1, h, w, l), v = XS(2, h, w, l);
    float sr = 0.f, su = 0.f, sv = 0.f;   // sum over the touched cells of g (2 f + eps g), in the order of the table
    if (cell(h, w, l)) {
      const float f2 = 2.f * FS(h, w, l);
      const float gr = -a.inv_dt + ((XS(1, h + 1, w, l) - u) + (XS(2, h, w + 1, l) - v)) * a.inv_dl - u * a.inv_dl - v * a.inv_dl;
      const float gu = -r * a.inv_dl + (XS(0, h + 1, w, l) - r) * a.inv_dl;
      const float gv = -r * a.inv_dl + (XS(0, h, w + 1, l) - r) * a.inv_dl;
      sr += gr * (f2 + a.eps * gr);
      su += gu * (f2 + a.eps * gu);
      sv += gv * (f2 + a.eps * gv);
    }
    if (cell(h, w, l - 1)) {
      const float g = a.inv_dt;
      sr += g * (2.f * FS(h, w, l - 1) + a.eps * g);
    }
    if (cell(h - 1, w, l)) {
      const float f2 = 2.f * FS(h - 1, w, l);
      const float gr = XS(1, h - 1, w, l) * a.inv_dl;
      const float gu = XS(0, h - 1, w, l) * a.inv_dl;
      sr += gr * (f2 + a.eps * gr);
      su += gu * (f2 + a.eps * gu);
    }
    if (cell(h, w - 1, l)) {
      const float f2 = 2.f * FS(h, w - 1, l);
      const float gr = XS(2, h, w - 1, l) * a.inv_dl;
      const float gv = XS(0, h, w - 1, l) * a.inv_dl;
      sr += gr * (f2 + a.eps * gr);
      sv += gv * (f2 + a.eps * gv);
    }
    const size_t o = ((size_t)h * W + w) * L + l;
    qb[o] = a.coef * sr;
    qb[HWL + o] = a.coef * su;
    qb[2 * HWL + o] = a.coef * sv;
    for (int c = 3; c < a.Cout; ++c) qb[c * HWL + o] = 0.f;
  }
#undef XS
#undef FS
}

hipError_t launch_mass_grad(const float *x, int Cin, float *q, int Cout, int B, int H, int W, int L, float delta_t,
                            float delta_l, float eps, hipStream_t st) {
  if (B <= 0 || H <= 0 || W <= 0 || L <= 0) return hipSuccess;
  MassGradArgs a{};
  a.x = x; a.Cin = Cin; a.q = q; a.Cout = Cout; a.H = H; a.W = W; a.L = L;
  // Whole rows of full W and L where they fit (the common case: bands of rows); otherwise halve the frame extent, then
  // the column extent, until a single row of the tile fits.  Rows per band: as many as fit, but no more than keep
  // ~512 workgroups in the grid (the kernel is latency-bound: at B = 32, 12 x 36 x 3, one row per band), split evenly.
  int tl = L, tw = W;
  while (mass_tile_floats(1, tw, tl) > kMassLdsFloats && tl > 1) tl = (tl + 1) / 2;
  while (mass_tile_floats(1, tw, tl) > kMassLdsFloats && tw > 1) tw = (tw + 1) / 2;
  int thmax = 1;
  while (thmax < H && mass_tile_floats(thmax + 1, tw, tl) <= kMassLdsFloats) ++thmax;
  const long long ntwl = (long long)((W + tw - 1) / tw) * ((L + tl - 1) / tl);
  const int thwant = (int)std::max(1LL, std::min((long long)thmax, ((long long)H * B * ntwl + 511) / 512));
  const int nth = (H + thwant - 1) / thwant;
  a.th = (H + nth - 1) / nth; a.tw = tw; a.tl = tl;
  a.nth = nth; a.ntw = (W + tw - 1) / tw; a.ntl = (L + tl - 1) / tl;
  a.inv_dt = (float)(1.0 / (double)delta_t);
  a.inv_dl = (float)(1.0 / (double)delta_l);
  a.eps = eps;
  a.coef = (float)(0.5 / ((double)H * W * L));
  const size_t lds = (size_t)mass_tile_floats(a.th, a.tw, a.tl) * sizeof(float);
  const long long blocks = (long long)B * a.nth * a.ntw * a.ntl;
  hipLaunchKernelGGL(mass_grad_kernel, dim3((unsigned)blocks), dim3(256), lds, st, a);
  return hipGetLastError();
}

// x[:, 0:3] -= c * q after the sampler step of the same step (ddpm.py:229: the product rounded, then the difference);
// like sampler_step_kernel it also rewrites the future frames of the channels-last UNet input and the history row.
__global__ __launch_bounds__(256) void mass_apply_kernel(MassApplyArgs a) {
  float c = a.c;
  float *hist = a.hist;
  if (a.tab) {
    const int k = *a.kctr;
    c = a.tab[k].mass;
    if (hist) hist += (long long)(k + 1) * a.row_stride + a.boff;
  }
  // 32-bit index math (the launcher checks that B * C * H * W * F fits)
  const int HWF = a.H * a.W * a.F;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.B * 3 * HWF) return;
  const int bc = i / HWF, s = i - bc * HWF;            // bc = b * 3 + ch; s = (h, w, f) within the channel
  const int b = bc / 3, ch = bc - b * 3;
  const int hw = s / a.F, f = s - hw * a.F;
  const int xi = (b * a.C + ch) * HWF + s;             // element of x [B][C][H][W][F]
  const float xn = __fsub_rn(a.x[xi], __fmul_rn(c, a.q[i]));
  a.x[xi] = xn;
  const int L = a.P + a.F;
  const int cl = (b * L + (a.P + f)) * (a.H * a.W) + hw;
  if (a.x8) a.x8[(size_t)cl * 8 + ch] = xn;
  if (hist) hist[xi] = xn;
}

hipError_t launch_mass_apply(const MassApplyArgs &a, hipStream_t st) {
  const long long total = (long long)a.B * 3 * a.H * a.W * a.F;
  if (total <= 0) return hipSuccess;
  if ((long long)a.B * (a.C > 3 ? a.C : 3) * a.H * a.W * (a.P + a.F) * 8 >= (1LL << 31)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(mass_apply_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a);
  return hipGetLastError();
}

}  // namespace cm
