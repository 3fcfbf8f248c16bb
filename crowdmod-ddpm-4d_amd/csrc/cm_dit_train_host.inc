// Training step of the DiT2D denoiser (arch "FM-DiT"), included at the end of cm_model.cpp.  Mirrors FM_model._train_step
// (models/flow_matching/flow_matching.py:104-157) below the host driver: u_pred = DiT2D(x_t, t, past) in train mode,
// loss = mse(u_pred, u_target), backward, torch.optim.Adam with coupled L2.  Kernels: cm_dit_train.hip, cm_dit.hip.
//
// Parameters, gradients and both Adam moments live in an OptStore (cm_opt_store.inc) whose frozen tensor is the sinusoid table
// (index 2 of the state_dict); the forward reads the master weights in place -- the DiT takes the reference layout, so an update
// leaves nothing to re-pack.  The eval path keeps its own weight copies and conditioning table (cm_dit_plan::w, modtab), which
// only cm_dit_train_sync refreshes.
//
// Tape, per block (allocated for max_batch by cm_dit_train_init): the residual stream entering the block and between its two
// halves (X cannot be updated in place), QKV, the attention's log-sum-exp and output, the pre-gate output of out_proj, the fc1
// pre-activation and the dropped fc2 output.  Recomputed in the backward: LayerNorm statistics with the normalised and the
// modulated rows, dropped GELU(fc1), every dropout mask, the attention probabilities, the patch matrix.
// The conditioning chain (time MLP, time_proj, both SiLUs, every adaLN_modulation.1) runs on the batch's B rows from the master
// weights of the step into mod [B][ldmod]; the forward GEMMs address it through an iota "timestep" buffer.

// The DiT4D_V4 denoiser (arch "DDPM-DiT", cm_dit4d_train_*) trains on the same state, entry-point bodies and backward halves; its
// forward, its temporal half and its tape are in cm_dit4d_train_host.inc.
struct cm_dit_train {
  OptStore opt;
  float dropout = 0.1f;
  int last_B = 0;
  long long sample_base = 0;
  std::vector<float *> Xs, QKV, AO, Yo, H1, Y2, LSE;   // tape: Xs[2 i] enters block i, Xs[2 i + 1] its MLP half
  std::vector<float *> QKVt, AOt, Yot, LSEt;           // DiT4D_V4: the temporal half's (Xs[3 i], Xs[3 i + 1], Xs[3 i + 2] there)
  float *Hm = nullptr, *G1 = nullptr, *G2 = nullptr, *GH = nullptr, *G3 = nullptr, *XN = nullptr, *Aln = nullptr, *rs = nullptr;
  float *dX = nullptr, *delta = nullptr, *Pm = nullptr, *dYf = nullptr, *pred = nullptr;
  float *mod = nullptr, *dmod = nullptr, *emb = nullptr, *h1 = nullptr, *h1s = nullptr, *e = nullptr, *z = nullptr, *c = nullptr;
  float *sc = nullptr, *dsc = nullptr, *dc = nullptr, *dz = nullptr, *de = nullptr, *dh1s = nullptr, *dh1 = nullptr;
  long long *iota = nullptr;
  float *wpart = nullptr;
  double *cpart = nullptr;       // float64 partials of the bias column sums
  float *mse_partial = nullptr, *mse_loss = nullptr;
  float *eps_dev = nullptr, *xt = nullptr;   // cm_dit4d_train_step: the drawn eps and q_sample's x_t [max_batch][C H W F]
  long long draws = 0;                       // eps draws so far (the Philox step word of the next one)
  // autocast (cm_dit4d_train_set_autocast; DiT4D_V4 only): f16 operands in the blocks' six token Linears, all three passes; the loss
  // gradient is multiplied by 2^ls_k and the flat gradient buffer by 2^-ls_k at the end of the backward
  int autocast = 0, ls_req = -1;             // mode; requested scale exponent (< 0: automatic)
  int ls_k = 0;                              // exponent of the step in flight (0 with the mode off)
  int ls_last_B = 0;                         // batch of the last autocast step (cm_dit4d_train_get_autocast)
};

void cm_free_dit_train(cm_dit_train *t) { delete t; }

namespace {

constexpr int DITT_KCHUNK = 256, DITT_MAX_SPLIT = 32;   // rows of one weight-gradient partial; partials per weight gradient

// `v4`: the cm_dit4d_train_* family, which takes DDPM-DiT (DiT4D_V4) handles only
int ditt_check(const cm_model *m, const char *what, bool need_train, bool v4 = false) {
  if (!m) return fail("%s: null model handle", what);
  if (v4) {
    if (!m->dit) return fail("%s: a UNet handle trains through cm_train_*; this entry point takes DDPM-DiT (DiT4D_V4) handles only", what);
    if (m->dit->full) return fail("%s: an FM-DiT (DiT2D) handle trains through cm_dit_train_*; this entry point takes DDPM-DiT (DiT4D_V4) handles only", what);
  } else {
    if (!m->dit) return fail("%s: a UNet handle trains through cm_train_*; this entry point takes FM-DiT (DiT2D) handles only", what);
    if (!m->dit->full) return fail("%s: DDPM-DiT (DiT4D_V4) training is not implemented; only FM-DiT (DiT2D) handles train", what);   // (here: cm_dit4d_train_*)
  }
  if (m->device < 0) return fail("%s: a host-only handle (device -1) cannot train", what);
  if (!m->finalized) return fail("%s: cm_model_finalize has not been called", what);
  if (m->precision != CM_PRECISION_F32)
    return fail("%s: training runs on fp32-plan handles: the f16 weight copies of an f16 sampling plan do not follow the optimizer", what);
  if (need_train && !m->dit->train) return fail("%s: %s has not been called", what, v4 ? "cm_dit4d_train_init" : "cm_dit_train_init");
  return 0;
}

int ditt4_forward(cm_model *m, int B, uint64_t seed, hipStream_t st);                           // cm_dit4d_train_host.inc
int ditt4_backward(cm_model *m, const float *d_target, int B, uint64_t seed, hipStream_t st);
int ditt4_scale_log2(const cm_model *m, int B);   // the loss-scale exponent of an autocast step at batch B

int ditt_setup(cm_model *m) {
  cm_dit_plan &d = *m->dit;
  cm_dit_train *T = d.train;
  const cm_dit_config &c = d.cfg;
  const size_t B = (size_t)c.max_batch, rows = B * d.tok, D = (size_t)c.hidden_size, mlp = (size_t)c.mlp_hidden;
  const size_t tx = D * c.time_multiple, F = sizeof(float);
  size_t maxw = 0, maxb = 1;
  for (const Param &p : m->params) {
    maxw = std::max(maxw, (size_t)p.numel());
    if (p.shape.size() == 1) maxb = std::max(maxb, (size_t)p.numel());
  }
  auto alloc = [&](float **p, size_t n) { return dev_alloc(m, (void **)p, n * F); };
  if (T->opt.init(m->params, {2}, false, alloc, d.w.data())) return 1;
  T->Xs.assign((d.full ? 2 : 3) * c.depth + 1, nullptr);
  for (float *&x : T->Xs) if (alloc(&x, rows * D)) return 1;
  for (auto *v : {&T->QKV, &T->AO, &T->Yo, &T->H1, &T->Y2, &T->LSE}) v->assign(c.depth, nullptr);
  for (int i = 0; i < c.depth; ++i) {
    if (alloc(&T->QKV[i], rows * 3 * D) || alloc(&T->AO[i], rows * D) || alloc(&T->Yo[i], rows * D) || alloc(&T->H1[i], rows * mlp) ||
        alloc(&T->Y2[i], rows * D) || alloc(&T->LSE[i], rows * c.num_heads))
      return 1;
  }
  if (!d.full) {   // the temporal half: its outputs are compact, the future slots' rows only
    const size_t frows = B * (size_t)(d.Tp - d.qs) * d.Ns;
    for (auto *v : {&T->QKVt, &T->AOt, &T->Yot, &T->LSEt}) v->assign(c.depth, nullptr);
    for (int i = 0; i < c.depth; ++i)
      if (alloc(&T->QKVt[i], rows * 3 * D) || alloc(&T->AOt[i], frows * D) || alloc(&T->Yot[i], frows * D) ||
          alloc(&T->LSEt[i], frows * c.num_heads))
        return 1;
    if (alloc(&T->eps_dev, B * (size_t)m->per_sample()) || alloc(&T->xt, B * (size_t)m->per_sample())) return 1;
  }
  if (alloc(&T->Hm, rows * mlp) || alloc(&T->GH, rows * mlp) || alloc(&T->G1, rows * D) || alloc(&T->G2, rows * D) ||
      alloc(&T->G3, rows * 3 * D) || alloc(&T->XN, rows * D) || alloc(&T->Aln, rows * D) || alloc(&T->rs, rows) ||
      alloc(&T->dX, rows * D) || alloc(&T->delta, rows * c.num_heads) || alloc(&T->Pm, rows * d.Kp) ||
      alloc(&T->dYf, rows * d.Nout) || alloc(&T->pred, B * (size_t)m->per_sample()))
    return 1;
  if (alloc(&T->mod, B * d.ldmod) || alloc(&T->dmod, B * d.ldmod) || alloc(&T->emb, B * D) || alloc(&T->h1, B * tx) ||
      alloc(&T->h1s, B * tx) || alloc(&T->e, B * tx) || alloc(&T->z, B * D) || alloc(&T->c, B * D) || alloc(&T->sc, B * D) ||
      alloc(&T->dsc, B * D) || alloc(&T->dc, B * D) || alloc(&T->dz, B * D) || alloc(&T->de, B * tx) || alloc(&T->dh1s, B * tx) ||
      alloc(&T->dh1, B * tx))
    return 1;
  if (dev_alloc(m, (void **)&T->cpart, (size_t)cm::DITT_COLSUM_SEGS * maxb * sizeof(double))) return 1;
  if (alloc(&T->wpart, (size_t)DITT_MAX_SPLIT * maxw) || alloc(&T->mse_partial, 64) || alloc(&T->mse_loss, 1)) return 1;
  std::vector<long long> io(B);
  std::iota(io.begin(), io.end(), 0LL);
  if (dev_alloc(m, (void **)&T->iota, B * sizeof(long long))) return 1;
  CM_HIP(hipMemcpy(T->iota, io.data(), B * sizeof(long long), hipMemcpyHostToDevice));
  CM_HIP(hipDeviceSynchronize());
  return 0;
}

// the conditioning rows of the batch from the master weights: e = time_blocks(t), c = SiLU(time_proj(e)), SiLU(c), every adaLN Linear
int ditt_conditioning(cm_model *m, int B, hipStream_t st) {
  const cm_dit_plan &d = *m->dit;
  cm_dit_train *T = d.train;
  const cm_dit_config &c = d.cfg;
  const int D = c.hidden_size, tx = D * c.time_multiple, nch = d.nchunk(), pb = d.per_block();
  auto W = [&](int i) { return T->opt.p + T->opt.off[i]; };
  auto lin = [&](const float *A, int K, int wi, float *Y, int N, int ldy) {
    cm::DitGemmArgs a = dit_gemm_args(cm::DIT_PRO_NONE, cm::DIT_EPI_BIAS, B, N, K);
    a.A = A; a.lda = K; a.W = W(wi); a.bias = W(wi + 1); a.Y = Y; a.ldy = ldy;
    return cm::launch_dit_gemm(a, st);
  };
  CM_HIP(cm::launch_ditt_gather_rows(W(2), m->tbuf, T->emb, B, D, st));
  CM_HIP(lin(T->emb, D, 3, T->h1, tx, tx));
  CM_HIP(cm::launch_ditt_silu(T->h1, T->h1s, nullptr, (long long)B * tx, st));
  CM_HIP(lin(T->h1s, tx, 5, T->e, tx, tx));
  CM_HIP(lin(T->e, tx, 7, T->z, D, D));
  CM_HIP(cm::launch_ditt_silu(T->z, T->c, nullptr, (long long)B * D, st));
  CM_HIP(cm::launch_ditt_silu(T->c, T->sc, nullptr, (long long)B * D, st));
  for (int i = 0; i <= c.depth; ++i) {
    const bool fin = i == c.depth;
    const int wi = fin ? DIT_HEAD + pb * c.depth + 2 : DIT_HEAD + pb * i + pb - 2;
    CM_HIP(lin(T->sc, D, wi, T->mod + (size_t)i * nch * D, fin ? 2 * D : nch * D, d.ldmod));
  }
  return 0;
}

// DiT2D.forward in train mode for the first B samples: x8, tbuf -> eps_cl, with the tape
int ditt_forward(cm_model *m, int B, uint64_t seed, hipStream_t st) {
  const cm_dit_plan &d = *m->dit;
  cm_dit_train *T = d.train;
  const cm_dit_config &c = d.cfg;
  const int D = c.hidden_size, D3 = 3 * D, mlp = c.mlp_hidden, nq = d.Tp - d.qs, nch = d.nchunk(), pb = d.per_block();
  const long long M = (long long)B * d.tok;
  auto W = [&](int i) { return T->opt.p + T->opt.off[i]; };
  cm::DitGemmArgs base{};
  base.tok = d.tok; base.tbuf = T->iota; base.mod = T->mod; base.ldmod = d.ldmod;
  base.L = m->L(); base.Hh = c.rows; base.Ww = c.cols; base.p = c.patch_size; base.pt = 1;
  base.Ns = d.Ns; base.wpn = c.cols / c.patch_size; base.Cout = c.out_channels;
  auto gemm = [&](int pro, int epi, long long rows, int N, int K) {
    cm::DitGemmArgs a = base;
    a.pro = pro; a.epi = epi; a.M = rows; a.N = N; a.K = K; a.grp = (int)rows;
    return a;
  };
  cm::DitDrop dr{seed, T->sample_base, T->opt.step, 0, T->dropout, 1};
  cm::DitGemmArgs a = gemm(cm::DIT_PRO_PATCH, cm::DIT_EPI_PATCH, M, D, d.Kp);
  a.x8 = m->x8; a.W = W(9); a.bias = W(10); a.Y = T->Xs[0]; a.ldy = D; a.spos = W(0); a.tpos = W(1);
  CM_HIP(cm::launch_dit_gemm(a, st));
  for (int i = 0; i < c.depth; ++i) {
    const int w0 = DIT_HEAD + pb * i, mo = i * nch * D;
    dr.block = i;
    float *Xin = T->Xs[2 * i], *Xmid = T->Xs[2 * i + 1], *Xout = T->Xs[2 * i + 2];
    a = gemm(cm::DIT_PRO_LN, cm::DIT_EPI_BIAS, M, D3, D);
    a.A = Xin; a.lda = D; a.W = W(w0); a.bias = W(w0 + 1); a.Y = T->QKV[i]; a.ldy = D3; a.off_shift = mo; a.off_scale = mo + D;
    CM_HIP(cm::launch_dit_gemm(a, st));
    cm::DitTrAttnArgs at{T->QKV[i], T->AO[i], T->LSE[i], nullptr, nullptr, nullptr, B, d.tok, D, c.num_heads, dr};
    CM_HIP(cm::launch_ditt_attn_fwd(at, st));
    a = gemm(cm::DIT_PRO_NONE, cm::DIT_EPI_BIAS, M, D, D);
    a.A = T->AO[i]; a.lda = D; a.W = W(w0 + 2); a.bias = W(w0 + 3); a.Y = T->Yo[i]; a.ldy = D;
    CM_HIP(cm::launch_dit_gemm(a, st));
    CM_HIP(cm::launch_ditt_gate(Xin, Xmid, T->Yo[i], nullptr, T->mod, d.ldmod, mo + 2 * D, M, D, d.tok, cm::DITT_SITE_NONE, dr, st));
    a = gemm(cm::DIT_PRO_LN, cm::DIT_EPI_BIAS, M, mlp, D);
    a.A = Xmid; a.lda = D; a.W = W(w0 + 4); a.bias = W(w0 + 5); a.Y = T->H1[i]; a.ldy = mlp; a.off_shift = mo + 3 * D; a.off_scale = mo + 4 * D;
    CM_HIP(cm::launch_dit_gemm(a, st));
    CM_HIP(cm::launch_ditt_gelu_drop(T->H1[i], T->Hm, M, mlp, d.tok, dr, 0, st));
    a = gemm(cm::DIT_PRO_NONE, cm::DIT_EPI_BIAS, M, D, mlp);
    a.A = T->Hm; a.lda = mlp; a.W = W(w0 + 6); a.bias = W(w0 + 7); a.Y = T->Y2[i]; a.ldy = D;
    CM_HIP(cm::launch_dit_gemm(a, st));
    CM_HIP(cm::launch_ditt_gate(Xmid, Xout, T->Y2[i], nullptr, T->mod, d.ldmod, mo + 5 * D, M, D, d.tok, cm::DITT_SITE_MLP2, dr, st));
  }
  const int wf = DIT_HEAD + pb * c.depth;
  a = gemm(cm::DIT_PRO_LN, cm::DIT_EPI_UNPATCH, M, d.Nout, D);
  a.M = (long long)B * nq * d.Ns; a.grp = nq * d.Ns; a.grp_stride = d.tok; a.grp_off = d.qs * d.Ns;
  a.A = T->Xs[2 * c.depth]; a.lda = D; a.W = W(wf); a.bias = W(wf + 1); a.Y = m->eps_cl;
  a.off_shift = c.depth * nch * D; a.off_scale = c.depth * nch * D + D;
  CM_HIP(cm::launch_dit_gemm(a, st));
  return 0;
}

// The backward's GEMMs, column sums and the state they run on, shared by both denoisers.
struct DittBwd {
  cm_model *m; cm_dit_train *T; hipStream_t st; int B;
  cm::DitTrLnArgs ln{};
  cm::DitTrPatchArgs pa{};
  cm::DitDrop dr{};
  float *W(int i) const { return T->opt.p + T->opt.off[i]; }
  float *G(int i) const { return T->opt.g + T->opt.off[i]; }
  // `tok`: the product belongs to one of a block's six token Linears, which take the f16-operand kernels in an autocast step
  // (the one place the backward picks them); the head, the patch embedding and the conditioning chain never pass it
  // dX [rows][Kin] (+)= dY [rows][Nout] W [Nout][Kin]
  hipError_t gemm_dx(const float *dY, int ldy, const float *Wm, float *dXo, long long rows, int Kin, int Nout, int accum,
                     bool tok = false) const {
    cm::DitTrGemmArgs g{dY, Wm, dXo, (int)rows, Kin, Nout, ldy, Kin, Kin, 0, accum, 1, 0, nullptr, tok && T->autocast};
    return cm::launch_ditt_gemm(g, st);
  }
  // dW [Nout][Kin] = dY^T A over `rows` rows, in fixed row ranges
  hipError_t gemm_dw(const float *dY, int ldy, const float *A, int lda, float *dW, long long rows, int Nout, int Kin,
                     bool tok = false) const {
    cm::DitTrGemmArgs g{dY, A, dW, Nout, Kin, rows, ldy, lda, Kin, 1, 0, 1, 0, nullptr, tok && T->autocast};
    long long ns = (rows + DITT_KCHUNK - 1) / DITT_KCHUNK;
    if (ns > 1) {
      ns = std::min<long long>(ns, DITT_MAX_SPLIT);
      g.nsplit = (int)ns; g.kchunk = ((rows + ns - 1) / ns + 31) / 32 * 32; g.part = T->wpart;
    }
    return cm::launch_ditt_gemm(g, st);
  }
  hipError_t colsum(const float *U, int ldu, float *out, long long rows, int N) const {
    return cm::launch_ditt_colsum(U, ldu, out, rows, N, T->cpart, st);
  }
};

// zeroed gradients, loss -> final layer (future rows only, compact); leaves ln set for the blocks (every row)
int ditt_bwd_head(DittBwd &o, const float *d_target, uint64_t seed) {
  cm_model *m = o.m;
  const cm_dit_plan &d = *m->dit;
  cm_dit_train *T = o.T;
  const cm_dit_config &c = d.cfg;
  hipStream_t st = o.st;
  const int B = o.B, D = c.hidden_size, nq = d.Tp - d.qs, nch = d.nchunk(), pb = d.per_block();
  const long long M = (long long)B * d.tok, Mf = (long long)B * nq * d.Ns;
  cm::DitTrLnArgs &ln = o.ln;
  ln.XN = T->XN; ln.A = T->Aln; ln.rs = T->rs; ln.dX = T->dX; ln.mod = T->mod; ln.ldmod = d.ldmod; ln.D = D; ln.tok = d.tok;
  o.dr = cm::DitDrop{seed, T->sample_base, T->opt.step, 0, T->dropout, 1};
  CM_HIP(hipMemsetAsync(T->opt.g, 0, T->opt.nfloats * sizeof(float), st));
  CM_HIP(hipMemsetAsync(T->dX, 0, (size_t)M * D * sizeof(float), st));

  cm::DitTrPatchArgs &pa = o.pa;
  pa.x8 = m->x8; pa.Pm = T->Pm; pa.pred = T->pred; pa.target = d_target; pa.dYf = T->dYf; pa.dX0 = T->dX;
  pa.dspos = o.G(0); pa.dtpos = o.G(1);
  pa.B = B; pa.C = c.out_channels; pa.L = m->L(); pa.Hh = c.rows; pa.Ww = c.cols; pa.p = c.patch_size; pa.Ns = d.Ns;
  pa.wpn = c.cols / c.patch_size; pa.tok = d.tok; pa.qs = d.qs; pa.Kp = d.Kp; pa.Nout = d.Nout; pa.D = D;
  pa.pt = c.t_patch_size; pa.P = c.past_len; pa.ls_k = T->ls_k;
  CM_HIP(cm::launch_ditt_loss_grad(pa, st));
  const int wf = DIT_HEAD + pb * c.depth, mof = c.depth * nch * D;
  ln.X = T->Xs.back(); ln.M = Mf; ln.grp = nq * d.Ns; ln.grp_stride = d.tok; ln.grp_off = d.qs * d.Ns;
  ln.off_shift = mof; ln.off_scale = mof + D; ln.dA = T->G1;
  CM_HIP(cm::launch_ditt_ln_fwd(ln, st));
  CM_HIP(o.gemm_dw(T->dYf, d.Nout, T->Aln, D, o.G(wf), Mf, d.Nout, D));
  CM_HIP(o.colsum(T->dYf, d.Nout, o.G(wf + 1), Mf, d.Nout));
  CM_HIP(o.gemm_dx(T->dYf, d.Nout, o.W(wf), T->G1, Mf, D, d.Nout, 0));
  CM_HIP(cm::launch_ditt_segsum(T->G1, D, nullptr, 0, T->dmod + mof, d.ldmod, B, (long long)nq * d.Ns, D, st));
  CM_HIP(cm::launch_ditt_segsum(T->G1, D, T->XN, D, T->dmod + mof + D, d.ldmod, B, (long long)nq * d.Ns, D, st));
  CM_HIP(cm::launch_ditt_ln_bwd(ln, st));
  ln.M = M; ln.grp = (int)M; ln.grp_stride = 0; ln.grp_off = 0;
  return 0;
}

// The gradient G [rows][N] of a Linear behind LayerNorm + modulate of X: its weight (index wi) and bias, the shift and scale
// chunks at mo, mo + D of d mod, and the residual-stream gradient.  `scratch`: [rows][D], not G.
int ditt_bwd_ln_linear(DittBwd &o, const float *X, const float *Gr, int N, int wi, int mo, float *scratch) {
  const cm_dit_plan &d = *o.m->dit;
  cm_dit_train *T = o.T;
  const int D = d.cfg.hidden_size;
  const long long M = (long long)o.B * d.tok;
  cm::DitTrLnArgs &ln = o.ln;
  ln.X = X; ln.off_shift = mo; ln.off_scale = mo + D; ln.dA = scratch;
  CM_HIP(cm::launch_ditt_ln_fwd(ln, o.st));
  CM_HIP(o.gemm_dw(Gr, N, T->Aln, D, o.G(wi), M, N, D, true));
  CM_HIP(o.colsum(Gr, N, o.G(wi + 1), M, N));
  CM_HIP(o.gemm_dx(Gr, N, o.W(wi), scratch, M, D, N, 0, true));
  CM_HIP(cm::launch_ditt_segsum(scratch, D, nullptr, 0, T->dmod + mo, d.ldmod, o.B, d.tok, D, o.st));
  CM_HIP(cm::launch_ditt_segsum(scratch, D, T->XN, D, T->dmod + mo + D, d.ldmod, o.B, d.tok, D, o.st));
  CM_HIP(cm::launch_ditt_ln_bwd(ln, o.st));
  return 0;
}

// MLP half of block i: x = x_mid + gate * drop2(fc2(drop1(gelu(fc1(modulate(LN(x_mid))))))); fc1 is tensor w, its chunks start at mo
int ditt_bwd_mlp(DittBwd &o, int i, const float *Xmid, int w, int mo) {
  const cm_dit_plan &d = *o.m->dit;
  cm_dit_train *T = o.T;
  hipStream_t st = o.st;
  const int B = o.B, D = d.cfg.hidden_size, mlp = d.cfg.mlp_hidden;
  const long long M = (long long)B * d.tok;
  CM_HIP(cm::launch_ditt_segsum(T->dX, D, T->Y2[i], D, T->dmod + mo + 2 * D, d.ldmod, B, d.tok, D, st));
  CM_HIP(cm::launch_ditt_gate(nullptr, nullptr, T->G1, T->dX, T->mod, d.ldmod, mo + 2 * D, M, D, d.tok, cm::DITT_SITE_MLP2, o.dr, st));
  CM_HIP(cm::launch_ditt_gelu_drop(T->H1[i], T->Hm, M, mlp, d.tok, o.dr, 0, st));
  CM_HIP(o.gemm_dw(T->G1, D, T->Hm, mlp, o.G(w + 2), M, D, mlp, true));
  CM_HIP(o.colsum(T->G1, D, o.G(w + 3), M, D));
  CM_HIP(o.gemm_dx(T->G1, D, o.W(w + 2), T->GH, M, mlp, D, 0, true));
  CM_HIP(cm::launch_ditt_gelu_drop(T->H1[i], T->GH, M, mlp, d.tok, o.dr, 1, st));
  return ditt_bwd_ln_linear(o, Xmid, T->GH, mlp, w, mo, T->G2);
}

// Self-attention half of block i over `groups` groups of S rows (DiT2D: the samples; DiT4D_V4: the (sample, slot) groups):
// x_mid = x_in + gate * out_proj(attention(in_proj(modulate(LN(x_in))))); in_proj is tensor w, its chunks start at mo
int ditt_bwd_attn(DittBwd &o, int i, const float *Xin, int w, int mo, int groups, int S) {
  const cm_dit_plan &d = *o.m->dit;
  cm_dit_train *T = o.T;
  hipStream_t st = o.st;
  const int B = o.B, D = d.cfg.hidden_size;
  const long long M = (long long)B * d.tok;
  CM_HIP(cm::launch_ditt_segsum(T->dX, D, T->Yo[i], D, T->dmod + mo + 2 * D, d.ldmod, B, d.tok, D, st));
  CM_HIP(cm::launch_ditt_gate(nullptr, nullptr, T->G1, T->dX, T->mod, d.ldmod, mo + 2 * D, M, D, d.tok, cm::DITT_SITE_NONE, o.dr, st));
  CM_HIP(o.gemm_dw(T->G1, D, T->AO[i], D, o.G(w + 2), M, D, D, true));
  CM_HIP(o.colsum(T->G1, D, o.G(w + 3), M, D));
  CM_HIP(o.gemm_dx(T->G1, D, o.W(w + 2), T->G2, M, D, D, 0, true));
  cm::DitDrop dr = o.dr;
  dr.gps = groups / B;
  cm::DitTrAttnArgs at{T->QKV[i], T->AO[i], T->LSE[i], T->G2, T->delta, T->G3, groups, S, D, d.cfg.num_heads, dr};
  CM_HIP(cm::launch_ditt_attn_delta(at, st));
  CM_HIP(cm::launch_ditt_attn_bwd(at, st));
  return ditt_bwd_ln_linear(o, Xin, T->G3, 3 * D, w, mo, T->G1);
}

// patch embedding and both position embeddings, then the conditioning chain: d mod [B][ldmod] through every adaLN Linear, the two
// SiLUs, time_proj and the time MLP
int ditt_bwd_tail(DittBwd &o) {
  const cm_dit_plan &d = *o.m->dit;
  cm_dit_train *T = o.T;
  const cm_dit_config &c = d.cfg;
  hipStream_t st = o.st;
  const int B = o.B, D = c.hidden_size, tx = D * c.time_multiple, nch = d.nchunk(), pb = d.per_block();
  const int wf = DIT_HEAD + pb * c.depth;
  const long long M = (long long)B * d.tok;
  CM_HIP(cm::launch_ditt_patch_gather(o.pa, st));
  CM_HIP(o.gemm_dw(T->dX, D, T->Pm, d.Kp, o.G(9), M, D, d.Kp));
  CM_HIP(o.colsum(T->dX, D, o.G(10), M, D));
  CM_HIP(cm::launch_ditt_pos_grad(o.pa, st));
  for (int i = 0; i <= c.depth; ++i) {
    const bool fin = i == c.depth;
    const int wi = fin ? wf + 2 : DIT_HEAD + pb * i + pb - 2, N = fin ? 2 * D : nch * D;
    const float *dm = T->dmod + (size_t)i * nch * D;
    CM_HIP(o.gemm_dw(dm, d.ldmod, T->sc, D, o.G(wi), B, N, D));
    CM_HIP(o.colsum(dm, d.ldmod, o.G(wi + 1), B, N));
    CM_HIP(o.gemm_dx(dm, d.ldmod, o.W(wi), T->dsc, B, D, N, i > 0));
  }
  CM_HIP(cm::launch_ditt_silu(T->c, T->dc, T->dsc, (long long)B * D, st));
  CM_HIP(cm::launch_ditt_silu(T->z, T->dz, T->dc, (long long)B * D, st));
  CM_HIP(o.gemm_dw(T->dz, D, T->e, tx, o.G(7), B, D, tx));
  CM_HIP(o.colsum(T->dz, D, o.G(8), B, D));
  CM_HIP(o.gemm_dx(T->dz, D, o.W(7), T->de, B, tx, D, 0));
  CM_HIP(o.gemm_dw(T->de, tx, T->h1s, tx, o.G(5), B, tx, tx));
  CM_HIP(o.colsum(T->de, tx, o.G(6), B, tx));
  CM_HIP(o.gemm_dx(T->de, tx, o.W(5), T->dh1s, B, tx, tx, 0));
  CM_HIP(cm::launch_ditt_silu(T->h1, T->dh1, T->dh1s, (long long)B * tx, st));
  CM_HIP(o.gemm_dw(T->dh1, tx, T->emb, D, o.G(3), B, tx, D));
  CM_HIP(o.colsum(T->dh1, tx, o.G(4), B, tx));
  return 0;
}

int ditt_backward(cm_model *m, const float *d_target, int B, uint64_t seed, hipStream_t st) {
  const cm_dit_plan &d = *m->dit;
  cm_dit_train *T = d.train;
  const int D = d.cfg.hidden_size, nch = d.nchunk(), pb = d.per_block();
  DittBwd o{m, T, st, B};
  if (ditt_bwd_head(o, d_target, seed)) return 1;
  for (int i = d.cfg.depth - 1; i >= 0; --i) {
    const int w0 = DIT_HEAD + pb * i, mo = i * nch * D;
    o.dr.block = i;
    if (ditt_bwd_mlp(o, i, T->Xs[2 * i + 1], w0 + 4, mo + 3 * D)) return 1;
    if (ditt_bwd_attn(o, i, T->Xs[2 * i], w0, mo, B, d.tok)) return 1;
  }
  return ditt_bwd_tail(o);
}

// ---- the bodies of the cm_dit_train_* / cm_dit4d_train_* entry points (`what`: the entry's name; `v4`: the DiT4D_V4 family) ----
int ditt_e_init(cm_model *m, const char *what, bool v4, float lr, float beta1, float beta2, float eps, float weight_decay,
                float dropout_rate) {
  if (ditt_check(m, what, false, v4)) return 1;
  if (!(dropout_rate >= 0.f && dropout_rate < 1.f)) return fail("%s: dropout rate %g outside [0,1)", what, dropout_rate);
  const cm_dit_config &c = m->dit->cfg;
  if (c.num_heads > 64 || c.depth > 8192 || m->dit->tok > 1024)
    return fail("%s: the dropout streams address at most 64 heads, 8192 blocks and 1024 tokens per sample", what);
  DevGuard g(m->device);
  if (!m->dit->train) {
    m->dit->train = new cm_dit_train();
    if (ditt_setup(m)) {   // no half-built state stays installed (the device buffers it got are cm_model::allocs')
      cm_free_dit_train(m->dit->train);
      m->dit->train = nullptr;
      return 1;
    }
  }
  m->dit->train->opt.hyper(lr, beta1, beta2, eps, weight_decay);
  m->dit->train->dropout = dropout_rate;
  return 0;
}

int ditt_e_set_sample_base(cm_model *m, const char *what, bool v4, int64_t sample_id_base) {
  if (ditt_check(m, what, true, v4)) return 1;
  if (sample_id_base < 0 || sample_id_base + m->cfg.max_batch > 0xffffffffLL)
    return fail("%s: sample indices must stay in [0, 2^32)", what);
  m->dit->train->sample_base = sample_id_base;
  return 0;
}

int ditt_e_step_xt(cm_model *m, const char *what, bool v4, const float *d_xt, const float *d_past, const int64_t *d_t,
                   const float *d_target, uint64_t seed, float *h_loss, int32_t B, int32_t apply_update, void *stream) {
  if (ditt_check(m, what, true, v4)) return 1;
  if (B < 1 || B > m->cfg.max_batch) return fail("%s: batch %d outside [1, max_batch=%d]", what, B, m->cfg.max_batch);
  if (!d_xt || !d_past || !d_t || !d_target || !h_loss) return fail("%s: null argument", what);
  DevGuard g(m->device);
  hipStream_t st = stream ? (hipStream_t)stream : m->stream;
  cm_dit_train *T = m->dit->train;
  const cm_unet_config &c = m->cfg;
  T->ls_k = T->autocast ? ditt4_scale_log2(m, B) : 0;
  if (T->autocast) T->ls_last_B = B;
  CM_HIP(hipMemcpyAsync(m->tbuf, d_t, (size_t)B * sizeof(long long), hipMemcpyDeviceToDevice, st));
  CM_HIP(cm::launch_assemble_input(d_past, d_xt, m->x8, B, c.in_channels, c.rows, c.cols, c.past_len, c.future_len, 3, st));
  if (ditt_conditioning(m, B, st) || (v4 ? ditt4_forward(m, B, seed, st) : ditt_forward(m, B, seed, st))) return 1;
  CM_HIP(cm::launch_extract_output(m->eps_cl, 8, T->pred, B, c.out_channels, c.rows, c.cols, c.past_len, c.future_len, st));
  CM_HIP(cm::launch_mse_loss(T->pred, d_target, (long long)B * m->per_sample(), T->mse_partial, T->mse_loss, st));
  T->last_B = B;
  if (v4 ? ditt4_backward(m, d_target, B, seed, st) : ditt_backward(m, d_target, B, seed, st)) return 1;
  if (apply_update && T->opt.apply(st)) return 1;
  CM_HIP(hipMemcpyAsync(h_loss, T->mse_loss, sizeof(float), hipMemcpyDeviceToHost, st));
  CM_HIP(hipStreamSynchronize(st));
  return 0;
}

int ditt_e_apply(cm_model *m, const char *what, bool v4, void *stream) {
  if (ditt_check(m, what, true, v4)) return 1;
  DevGuard g(m->device);
  hipStream_t st = stream ? (hipStream_t)stream : m->stream;
  if (m->dit->train->opt.apply(st)) return 1;
  CM_HIP(hipStreamSynchronize(st));
  return 0;
}

int ditt_e_get_grad(cm_model *m, const char *what, bool v4, const char *name, float *h_out, int64_t numel) {
  if (ditt_check(m, what, true, v4)) return 1;
  DevGuard g(m->device);
  return m->dit->train->opt.copy_out(m->params, m->dit->train->opt.g, name, numel, h_out);
}

// which: 0 exp_avg, 1 exp_avg_sq, and on get only 2 the master weights themselves
int ditt_e_get_opt_state(cm_model *m, const char *what, bool v4, const char *name, int32_t which, float *h_out, int64_t numel) {
  if (ditt_check(m, what, true, v4)) return 1;
  if (which < 0 || which > 2) return fail("%s: optimizer state %d: 0 = exp_avg, 1 = exp_avg_sq, 2 = master weights", what, which);
  DevGuard g(m->device);
  OptStore &S = m->dit->train->opt;
  return S.copy_out(m->params, which == 0 ? S.m : which == 1 ? S.v : S.p, name, numel, h_out);
}

int ditt_e_set_opt_state(cm_model *m, const char *what, bool v4, const char *name, int32_t which, const float *h_in, int64_t numel) {
  if (ditt_check(m, what, true, v4)) return 1;
  if (which < 0 || which > 1) return fail("%s: optimizer state %d: 0 = exp_avg, 1 = exp_avg_sq", what, which);
  DevGuard g(m->device);
  OptStore &S = m->dit->train->opt;
  return S.copy_in(m->params, which ? S.v : S.m, name, numel, h_in);
}

// The master weights into the handle's state_dict and into the eval path's weight copies, and the 1000-row conditioning table
// rebuilt from them: until this call the eval forward computes what it computed before training.
int ditt_e_sync(cm_model *m, const char *what, bool v4) {
  if (ditt_check(m, what, true, v4)) return 1;
  DevGuard g(m->device);
  cm_dit_plan &d = *m->dit;
  cm_dit_train *T = d.train;
  if (T->opt.pull_masters(m->params)) return 1;
  for (size_t i = 0; i < m->params.size(); ++i)
    CM_HIP(hipMemcpy(const_cast<float *>(d.w[i]), T->opt.p + T->opt.off[i], (size_t)m->params[i].numel() * sizeof(float), hipMemcpyDeviceToDevice));
  return dit_build_tables(m);
}

int ditt_e_get_pred(cm_model *m, const char *what, bool v4, float *h_out, int64_t numel) {
  if (ditt_check(m, what, true, v4)) return 1;
  cm_dit_train *T = m->dit->train;
  if (!h_out) return fail("%s: null argument", what);
  if (T->last_B < 1) return fail("%s: no training step has run", what);
  if (numel != (int64_t)T->last_B * m->per_sample()) return fail("%s: %lld elements, the last step predicted %lld", what, (long long)numel, (long long)T->last_B * m->per_sample());
  DevGuard g(m->device);
  CM_HIP(hipMemcpy(h_out, T->pred, (size_t)numel * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}

}  // namespace

extern "C" {

int cm_dit_train_init(cm_model *m, float lr, float beta1, float beta2, float eps, float weight_decay, float dropout_rate) {
  return ditt_e_init(m, "cm_dit_train_init", false, lr, beta1, beta2, eps, weight_decay, dropout_rate);
}

int cm_dit_train_set_lr(cm_model *m, float lr) {
  if (ditt_check(m, "cm_dit_train_set_lr", true)) return 1;
  m->dit->train->opt.lr = lr;
  return 0;
}

int cm_dit_train_set_sample_base(cm_model *m, int64_t sample_id_base) {
  return ditt_e_set_sample_base(m, "cm_dit_train_set_sample_base", false, sample_id_base);
}

int cm_dit_train_step_xt(cm_model *m, const float *d_xt, const float *d_past, const int64_t *d_t, const float *d_target, uint64_t seed,
                         float *h_loss, int32_t B, int32_t apply_update, void *stream) {
  return ditt_e_step_xt(m, "cm_dit_train_step_xt", false, d_xt, d_past, d_t, d_target, seed, h_loss, B, apply_update, stream);
}

int cm_dit_train_flat_grads(cm_model *m, void **d_grads, int64_t *numel) {
  if (ditt_check(m, "cm_dit_train_flat_grads", true)) return 1;
  return m->dit->train->opt.flat_grads(d_grads, numel);
}

int cm_dit_train_apply(cm_model *m, void *stream) { return ditt_e_apply(m, "cm_dit_train_apply", false, stream); }

int cm_dit_train_get_grad(cm_model *m, const char *name, float *h_out, int64_t numel) {
  return ditt_e_get_grad(m, "cm_dit_train_get_grad", false, name, h_out, numel);
}

int cm_dit_train_get_opt_state(cm_model *m, const char *name, int32_t which, float *h_out, int64_t numel) {
  return ditt_e_get_opt_state(m, "cm_dit_train_get_opt_state", false, name, which, h_out, numel);
}

int cm_dit_train_set_opt_state(cm_model *m, const char *name, int32_t which, const float *h_in, int64_t numel) {
  return ditt_e_set_opt_state(m, "cm_dit_train_set_opt_state", false, name, which, h_in, numel);
}

int cm_dit_train_opt_step(cm_model *m, int32_t *step, int32_t set) {
  if (ditt_check(m, "cm_dit_train_opt_step", true)) return 1;
  return m->dit->train->opt.opt_step(step, set);
}

int cm_dit_train_sync(cm_model *m) { return ditt_e_sync(m, "cm_dit_train_sync", false); }

int cm_dit_train_get_pred(cm_model *m, float *h_out, int64_t numel) {
  return ditt_e_get_pred(m, "cm_dit_train_get_pred", false, h_out, numel);
}

}  // extern "C"

#include "cm_dit4d_train_host.inc"
