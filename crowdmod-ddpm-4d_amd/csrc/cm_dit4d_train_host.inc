// Training step of the DiT4D_V4 denoiser (arch "DDPM-DiT"), included by cm_dit_train_host.inc at the end of cm_model.cpp.  Mirrors
// DDPM_model._train_step (models/diffusion/ddpm.py:111-154) below the host driver: eps_hat = DiT4D_V4(x_t, t, past) in train mode
// (models/backbones/DiT4D_V4.py:106-204, 347-375), loss = mse(eps_hat, eps), backward, torch.optim.Adam with coupled L2; fp32
// unless cm_dit4d_train_set_autocast puts the blocks' six token Linears on f16 operands (the reference's torch.amp.autocast,
// ddpm.py:116-120).  Kernels: cm_dit4d_train.hip, cm_dit_train.hip, cm_dit.hip.
//
// The state (cm_dit_train), the OptStore with the sinusoid table frozen, the conditioning chain (9 depth + 2 chunks), the final
// layer, the MLP half, the patch / position embeddings and the entry-point bodies are cm_dit_train_host.inc's.  What is here is
// the block structure:
//   spatial half    ditt_attn_* with one (sample, slot) group of N_s rows as the kernels' "sample" (B T_p groups; DitDrop::gps =
//                   T_p gives the masks their real coordinates), gated residual on every row
//   temporal half   ditt4_tattn_* per (sample, patch); in-projection on every row, output, out-projection and the gated residual
//                   on the future slots' rows only (compact [B][(T_p - qs) N_s][D]); past rows pass through
// Tape per block, over DiT2D's: the residual stream after the spatial half too (Xs[3 i .. 3 i + 2]), and the temporal half's QKV,
// lse, output and pre-gate out-projection.

namespace {

int ditt4_forward(cm_model *m, int B, uint64_t seed, hipStream_t st) {
  const cm_dit_plan &d = *m->dit;
  cm_dit_train *T = d.train;
  const cm_dit_config &c = d.cfg;
  const int D = c.hidden_size, D3 = 3 * D, mlp = c.mlp_hidden, nq = d.Tp - d.qs, nch = d.nchunk(), pb = d.per_block();
  const long long M = (long long)B * d.tok, Mf = (long long)B * nq * d.Ns;
  auto W = [&](int i) { return T->opt.p + T->opt.off[i]; };
  cm::DitGemmArgs base{};
  base.tok = d.tok; base.tbuf = T->iota; base.mod = T->mod; base.ldmod = d.ldmod;
  base.L = m->L(); base.Hh = c.rows; base.Ww = c.cols; base.p = c.patch_size; base.pt = c.t_patch_size;
  base.Ns = d.Ns; base.wpn = c.cols / c.patch_size; base.Cout = c.out_channels;
  auto gemm = [&](int pro, int epi, long long rows, int N, int K) {
    cm::DitGemmArgs a = base;
    a.pro = pro; a.epi = epi; a.M = rows; a.N = N; a.K = K; a.grp = (int)rows;
    return a;
  };
  // a token Linear of a block (bias epilogue): the one place the forward picks the f16-operand form of an autocast step
  auto linear = [&](int pro, long long rows, int N, int K) {
    cm::DitGemmArgs a = gemm(pro, cm::DIT_EPI_BIAS, rows, N, K);
    a.f16 = T->autocast;
    return a;
  };
  cm::DitDrop dr{seed, T->sample_base, T->opt.step, 0, T->dropout, 1};
  cm::DitGemmArgs a = gemm(cm::DIT_PRO_PATCH, cm::DIT_EPI_PATCH, M, D, d.Kp);
  a.x8 = m->x8; a.W = W(9); a.bias = W(10); a.Y = T->Xs[0]; a.ldy = D; a.spos = W(0); a.tpos = W(1);
  CM_HIP(cm::launch_dit_gemm(a, st));
  for (int i = 0; i < c.depth; ++i) {
    const int w0 = DIT_HEAD + pb * i, mo = i * nch * D;
    dr.block = i;
    float *Xin = T->Xs[3 * i], *Xsp = T->Xs[3 * i + 1], *Xtm = T->Xs[3 * i + 2], *Xout = T->Xs[3 * i + 3];
    // spatial self-attention per (sample, slot) (DiT4D_V4.py:160-169)
    a = linear(cm::DIT_PRO_LN, M, D3, D);
    a.A = Xin; a.lda = D; a.W = W(w0); a.bias = W(w0 + 1); a.Y = T->QKV[i]; a.ldy = D3; a.off_shift = mo; a.off_scale = mo + D;
    CM_HIP(cm::launch_dit_gemm(a, st));
    cm::DitDrop ds = dr;
    ds.gps = d.Tp;
    cm::DitTrAttnArgs at{T->QKV[i], T->AO[i], T->LSE[i], nullptr, nullptr, nullptr, B * d.Tp, d.Ns, D, c.num_heads, ds};
    CM_HIP(cm::launch_ditt_attn_fwd(at, st));
    a = linear(cm::DIT_PRO_NONE, M, D, D);
    a.A = T->AO[i]; a.lda = D; a.W = W(w0 + 2); a.bias = W(w0 + 3); a.Y = T->Yo[i]; a.ldy = D;
    CM_HIP(cm::launch_dit_gemm(a, st));
    CM_HIP(cm::launch_ditt_gate(Xin, Xsp, T->Yo[i], nullptr, T->mod, d.ldmod, mo + 2 * D, M, D, d.tok, cm::DITT_SITE_NONE, dr, st));
    // temporal cross-attention per (sample, patch): keys / values every slot, queries and the residual the slots >= qs (:173-198)
    a = linear(cm::DIT_PRO_LN, M, D3, D);
    a.A = Xsp; a.lda = D; a.W = W(w0 + 4); a.bias = W(w0 + 5); a.Y = T->QKVt[i]; a.ldy = D3; a.off_shift = mo + 3 * D; a.off_scale = mo + 4 * D;
    CM_HIP(cm::launch_dit_gemm(a, st));
    cm::DitTrTAttnArgs tt{T->QKVt[i], T->AOt[i], T->LSEt[i], nullptr, nullptr, B, d.Tp, d.Ns, d.qs, D, c.num_heads, dr};
    CM_HIP(cm::launch_ditt4_tattn_fwd(tt, st));
    a = linear(cm::DIT_PRO_NONE, Mf, D, D);
    a.A = T->AOt[i]; a.lda = D; a.W = W(w0 + 6); a.bias = W(w0 + 7); a.Y = T->Yot[i]; a.ldy = D;
    CM_HIP(cm::launch_dit_gemm(a, st));
    CM_HIP(cm::launch_ditt4_gate_rows(Xsp, Xtm, T->Yot[i], nullptr, nullptr, T->mod, d.ldmod, mo + 5 * D, B, d.tok, d.qs * d.Ns, D, st));
    // MLP (:201-202)
    a = linear(cm::DIT_PRO_LN, M, mlp, D);
    a.A = Xtm; a.lda = D; a.W = W(w0 + 8); a.bias = W(w0 + 9); a.Y = T->H1[i]; a.ldy = mlp; a.off_shift = mo + 6 * D; a.off_scale = mo + 7 * D;
    CM_HIP(cm::launch_dit_gemm(a, st));
    CM_HIP(cm::launch_ditt_gelu_drop(T->H1[i], T->Hm, M, mlp, d.tok, dr, 0, st));
    a = linear(cm::DIT_PRO_NONE, M, D, mlp);
    a.A = T->Hm; a.lda = mlp; a.W = W(w0 + 10); a.bias = W(w0 + 11); a.Y = T->Y2[i]; a.ldy = D;
    CM_HIP(cm::launch_dit_gemm(a, st));
    CM_HIP(cm::launch_ditt_gate(Xtm, Xout, T->Y2[i], nullptr, T->mod, d.ldmod, mo + 8 * D, M, D, d.tok, cm::DITT_SITE_MLP2, dr, st));
  }
  // final layer + unpatchify on the future slots' rows (:223-225, :93-99)
  const int wf = DIT_HEAD + pb * c.depth;
  a = gemm(cm::DIT_PRO_LN, cm::DIT_EPI_UNPATCH, M, d.Nout, D);
  a.M = Mf; a.grp = nq * d.Ns; a.grp_stride = d.tok; a.grp_off = d.qs * d.Ns;
  a.A = T->Xs[3 * c.depth]; a.lda = D; a.W = W(wf); a.bias = W(wf + 1); a.Y = m->eps_cl;
  a.off_shift = c.depth * nch * D; a.off_scale = c.depth * nch * D + D;
  CM_HIP(cm::launch_dit_gemm(a, st));
  return 0;
}

// temporal half of block i: x_tm = x_sp + [rows >= qs N_s] gate2 * out_proj(attention(in_proj(modulate(LN(x_sp)))))
int ditt4_bwd_temporal(DittBwd &o, int i, const float *Xsp, int w, int mo) {
  const cm_dit_plan &d = *o.m->dit;
  cm_dit_train *T = o.T;
  hipStream_t st = o.st;
  const int B = o.B, D = d.cfg.hidden_size, nq = d.Tp - d.qs, row0 = d.qs * d.Ns;
  const long long Mf = (long long)B * nq * d.Ns;
  // d gate2 = sum over the future rows of dX * attn_t; the residual's own gradient stays in dX on every row
  CM_HIP(cm::launch_ditt_segsum_rows(T->dX + (size_t)row0 * D, D, d.tok, T->Yot[i], D, (long long)nq * d.Ns, T->dmod + mo + 2 * D, d.ldmod,
                                     B, (long long)nq * d.Ns, D, st));
  CM_HIP(cm::launch_ditt4_gate_rows(nullptr, nullptr, nullptr, T->G1, T->dX, T->mod, d.ldmod, mo + 2 * D, B, d.tok, row0, D, st));
  CM_HIP(o.gemm_dw(T->G1, D, T->AOt[i], D, o.G(w + 2), Mf, D, D, true));
  CM_HIP(o.colsum(T->G1, D, o.G(w + 3), Mf, D));
  CM_HIP(o.gemm_dx(T->G1, D, o.W(w + 2), T->G2, Mf, D, D, 0, true));
  cm::DitTrTAttnArgs tt{T->QKVt[i], nullptr, T->LSEt[i], T->G2, T->G3, B, d.Tp, d.Ns, d.qs, D, d.cfg.num_heads, o.dr};
  CM_HIP(cm::launch_ditt4_tattn_bwd(tt, st));
  return ditt_bwd_ln_linear(o, Xsp, T->G3, 3 * D, w, mo, T->G1);
}

int ditt4_backward(cm_model *m, const float *d_target, int B, uint64_t seed, hipStream_t st) {
  const cm_dit_plan &d = *m->dit;
  cm_dit_train *T = d.train;
  const int D = d.cfg.hidden_size, nch = d.nchunk(), pb = d.per_block();
  DittBwd o{m, T, st, B};
  if (ditt_bwd_head(o, d_target, seed)) return 1;
  for (int i = d.cfg.depth - 1; i >= 0; --i) {
    const int w0 = DIT_HEAD + pb * i, mo = i * nch * D;
    o.dr.block = i;
    if (ditt_bwd_mlp(o, i, T->Xs[3 * i + 2], w0 + 8, mo + 6 * D)) return 1;
    if (ditt4_bwd_temporal(o, i, T->Xs[3 * i + 1], w0 + 4, mo + 3 * D)) return 1;
    if (ditt_bwd_attn(o, i, T->Xs[3 * i], w0, mo, B * d.Tp, d.Ns)) return 1;
  }
  if (ditt_bwd_tail(o)) return 1;
  // autocast: every gradient above carries the loss scale 2^k exactly (fp32 tensors); take it out once, so that the readers of the
  // flat buffer (cm_dit4d_train_get_grad, flat_grads and the all-reduce, Adam, checkpoints) see unscaled gradients
  if (T->ls_k > 0) CM_HIP(cm::launch_scale_inplace(T->opt.g, (long long)T->opt.nfloats, ldexpf(1.f, -T->ls_k), st));
  return 0;
}

// the requested exponent, or the largest k with 2^k <= B*C*H*W*F (loss gradient O(1)): a function of B alone
int ditt4_scale_log2(const cm_model *m, int B) { return loss_scale_log2(m->dit->train->ls_req, (long long)B * m->per_sample()); }

}  // namespace

extern "C" {

int cm_dit4d_train_init(cm_model *m, float lr, float beta1, float beta2, float eps, float weight_decay, float dropout_rate) {
  return ditt_e_init(m, "cm_dit4d_train_init", true, lr, beta1, beta2, eps, weight_decay, dropout_rate);
}

int cm_dit4d_train_set_lr(cm_model *m, float lr) {
  if (ditt_check(m, "cm_dit4d_train_set_lr", true, true)) return 1;
  m->dit->train->opt.lr = lr;
  return 0;
}

// The reference wraps DDPM_model._train_step in torch.amp.autocast without a GradScaler (ddpm.py:116-120), whatever the denoiser.
// The fp32 master weights are read and rounded while staging, so no f16 copy exists that an update, cm_dit4d_train_set_opt_state,
// a loaded checkpoint or cm_dit4d_train_sync could leave stale.
int cm_dit4d_train_set_autocast(cm_model *m, int32_t mode, int32_t loss_scale_log2) {
  if (ditt_check(m, "cm_dit4d_train_set_autocast", true, true)) return 1;
  if (mode != 0 && mode != 1) return fail("cm_dit4d_train_set_autocast: mode %d: 0 = fp32 step, 1 = autocast", (int)mode);
  if (loss_scale_log2 > 24) return fail("cm_dit4d_train_set_autocast: loss_scale_log2 %d above 24", (int)loss_scale_log2);
  cm_dit_train *T = m->dit->train;
  T->autocast = mode; T->ls_req = mode ? (int)loss_scale_log2 : -1;
  if (T->ls_req < 0) T->ls_req = -1;
  return 0;
}

int cm_dit4d_train_get_autocast(const cm_model *m, int32_t *mode, int32_t *loss_scale_log2) {
  if (ditt_check(m, "cm_dit4d_train_get_autocast", true, true)) return 1;
  if (!mode || !loss_scale_log2) return fail("cm_dit4d_train_get_autocast: null argument");
  const cm_dit_train *T = m->dit->train;
  *mode = T->autocast;
  *loss_scale_log2 = T->autocast ? ditt4_scale_log2(m, T->ls_last_B > 0 ? T->ls_last_B : m->cfg.max_batch) : 0;
  return 0;
}

int cm_dit4d_train_set_sample_base(cm_model *m, int64_t sample_id_base) {
  return ditt_e_set_sample_base(m, "cm_dit4d_train_set_sample_base", true, sample_id_base);
}

int cm_dit4d_train_step_xt(cm_model *m, const float *d_xt, const float *d_past, const int64_t *d_t, const float *d_target, uint64_t seed,
                           float *h_loss, int32_t B, int32_t apply_update, void *stream) {
  return ditt_e_step_xt(m, "cm_dit4d_train_step_xt", true, d_xt, d_past, d_t, d_target, seed, h_loss, B, apply_update, stream);
}

// cm_train_step's shape: x_t = q_sample(future, t, eps), target eps; a null d_eps draws eps with cm_train_step's addressing (one
// substream per (draw, global sample))
int cm_dit4d_train_step(cm_model *m, const cm_schedule *s, const float *d_future, const float *d_past, const int64_t *d_t,
                        const float *d_eps, uint64_t seed, float *h_loss, int32_t B, int32_t apply_update, void *stream) {
  if (ditt_check(m, "cm_dit4d_train_step", true, true)) return 1;
  if (B < 1 || B > m->cfg.max_batch) return fail("cm_dit4d_train_step: batch %d outside [1, max_batch=%d]", B, m->cfg.max_batch);
  if (!s || !d_future || !d_past || !d_t || !h_loss) return fail("cm_dit4d_train_step: null argument");
  cm_dit_train *T = m->dit->train;
  const long long per = (long long)m->per_sample();
  {
    DevGuard g(m->device);
    hipStream_t st = stream ? (hipStream_t)stream : m->stream;
    if (!d_eps) {
      CM_HIP(cm::launch_randn(T->eps_dev, B, per, seed, T->sample_base, 0x40000000 + (int)(T->draws & 0x3fffffff), st));
      T->draws += 1;
      d_eps = T->eps_dev;
    }
    CM_HIP(cm::launch_q_sample(d_future, (const long long *)d_t, d_eps, s->d_sab, s->d_s1m, T->xt, B, per, st));
  }
  return ditt_e_step_xt(m, "cm_dit4d_train_step", true, T->xt, d_past, d_t, d_eps, seed, h_loss, B, apply_update, stream);
}

int cm_dit4d_train_flat_grads(cm_model *m, void **d_grads, int64_t *numel) {
  if (ditt_check(m, "cm_dit4d_train_flat_grads", true, true)) return 1;
  return m->dit->train->opt.flat_grads(d_grads, numel);
}

int cm_dit4d_train_apply(cm_model *m, void *stream) { return ditt_e_apply(m, "cm_dit4d_train_apply", true, stream); }

int cm_dit4d_train_get_grad(cm_model *m, const char *name, float *h_out, int64_t numel) {
  return ditt_e_get_grad(m, "cm_dit4d_train_get_grad", true, name, h_out, numel);
}

int cm_dit4d_train_get_opt_state(cm_model *m, const char *name, int32_t which, float *h_out, int64_t numel) {
  return ditt_e_get_opt_state(m, "cm_dit4d_train_get_opt_state", true, name, which, h_out, numel);
}

int cm_dit4d_train_set_opt_state(cm_model *m, const char *name, int32_t which, const float *h_in, int64_t numel) {
  return ditt_e_set_opt_state(m, "cm_dit4d_train_set_opt_state", true, name, which, h_in, numel);
}

int cm_dit4d_train_opt_step(cm_model *m, int32_t *step, int32_t set) {
  if (ditt_check(m, "cm_dit4d_train_opt_step", true, true)) return 1;
  return m->dit->train->opt.opt_step(step, set);
}

int cm_dit4d_train_sync(cm_model *m) { return ditt_e_sync(m, "cm_dit4d_train_sync", true); }

int cm_dit4d_train_get_pred(cm_model *m, float *h_out, int64_t numel) {
  return ditt_e_get_pred(m, "cm_dit4d_train_get_pred", true, h_out, numel);
}

}  // extern "C"
