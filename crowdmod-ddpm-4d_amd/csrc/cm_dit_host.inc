// Host plan of the DiT4D_V4 denoiser (models/backbones/DiT4D_V4.py), included by cm_model.cpp.  A DiT handle is a
// cm_model with `dit` set: the shared code (cm_sample_loop, the host-buffer variants, cm_unet_forward's layout change)
// sees the sampler geometry through cm_model::cfg and calls denoise(), which runs dit_forward instead of run_ops.
// Kernels: cm_dit.hip.  Nothing here writes plan state at launch time: the two batch lanes of cm_sample_loop enqueue
// dit_forward from two host threads on disjoint workspace rows.
//
// The DiT2D denoiser of arch "FM-DiT" (models/backbones/DiT2D.py) is the same plan with `full` set: t_patch_size 1 (its
// per-frame Conv2d patchify is the Conv3d gather with one frame per slot, weight order (C, p, p), token order (frame,
// h_p, w_p); its unpatchify is the scatter with pt = 1), one self-attention over all T_p * N_s tokens per block instead
// of the spatial / temporal pair, 6 modulation chunks per block instead of 9, and 10 tensors per block instead of 14.

struct cm_dit_train;                       // cm_dit_train_host.inc: the training state of a DiT2D handle (cm_dit_train_init)
void cm_free_dit_train(cm_dit_train *t);   // (host-side struct only; its device buffers live in cm_model::allocs)
struct cm_dit_plan {
  ~cm_dit_plan() { cm_free_dit_train(train); }
  cm_dit_train *train = nullptr;
  cm_dit_config cfg{};
  bool full = false;           // DiT2D: one full self-attention per block (cm_model_create_dit2d)
  int Ns = 0, Tp = 0, qs = 0, tok = 0, Kp = 0, Nout = 0, ldmod = 0;
  int nchunk() const { return full ? 6 : 9; }                  // modulation chunks per block
  int per_block() const { return full ? 10 : 14; }             // state_dict tensors per block
  float *X = nullptr, *QKV = nullptr, *AO = nullptr, *Hm = nullptr;   // [max_batch * tok][D | 3D | D | mlp_hidden]
  float *modtab = nullptr;     // [1000][depth * 9D + 2D]: per block shift1 scale1 gate1 shift2 ... gate3, then the final layer's
                               // (DiT2D: depth * 6D + 2D, shift1 scale1 gate1 shift2 scale2 gate2)
  float *tab_h1 = nullptr, *tab_e = nullptr, *tab_cs = nullptr;   // scratch of dit_build_tables
  std::vector<const float *> w;  // device copies of the state_dict tensors, in state_dict order
  std::vector<const _Float16 *> w16;   // f16 plans (cm_model::precision == CM_PRECISION_F16 on DiT4D_V4, CM_PRECISION_F16A on DiT2D): per
                               // tensor of `w`, its copy rounded once to f16 (cm_dit_f16.h), same [out][in] order -- the six (DiT2D: four)
                               // token-Linear weights of every block; null elsewhere.  Empty on the fp32 plan.  Written by dit_finalize,
                               // read-only afterwards.
  bool attn16() const { return full && !w16.empty(); }   // f16a plan: the full attention takes dit_attn_full_f16_kernel
};

namespace {

// state_dict order of DiT4D_V4: own parameters first (spatial_pos_embed, temporal_pos_embed: DiT4D_V4.py:289-295), then the
// child modules in registration order (dif_time_embeddings, time_proj, patch_embed, blocks, final_layer).
constexpr int DIT_HEAD = 11;     // tensors before blocks.0 (both variants)
// f16 plan: the weights of a DiT4D_V4 block (dit_build_params order) that get an f16 copy -- spatial in_proj, spatial out_proj,
// temporal in_proj, temporal out_proj, mlp.0, mlp.3
constexpr int DIT_F16_W[6] = {0, 2, 4, 6, 8, 10};
// f16a plan: those of a DiT2D block (dit2d_build_params order) -- attn.in_proj_weight, attn.out_proj.weight, mlp.0.weight, mlp.3.weight
constexpr int DIT2D_F16_W[4] = {0, 2, 4, 6};

// state_dict order of DiT2D: spatial_pos_embed, temporal_pos_embed (DiT2D.py:196-201 -- registered after time_embeddings
// and patch_embed, but a module's own parameters come first), then time_embeddings, time_proj, patch_embed, blocks,
// final_layer.
void dit2d_build_params(cm_model *m) {
  const cm_dit_config &c = m->dit->cfg;
  const int64_t D = c.hidden_size, tx = D * c.time_multiple, p = c.patch_size;
  add_param(m, "spatial_pos_embed", {1, m->dit->Ns, D});
  add_param(m, "temporal_pos_embed", {1, c.t_max, D});
  add_param(m, "time_embeddings.time_blocks.0.weight", {TIME_ROWS, D});
  add_param(m, "time_embeddings.time_blocks.1.weight", {tx, D});
  add_param(m, "time_embeddings.time_blocks.1.bias", {tx});
  add_param(m, "time_embeddings.time_blocks.3.weight", {tx, tx});
  add_param(m, "time_embeddings.time_blocks.3.bias", {tx});
  add_param(m, "time_proj.0.weight", {D, tx});
  add_param(m, "time_proj.0.bias", {D});
  add_param(m, "patch_embed.proj.weight", {D, c.in_channels, p, p});
  add_param(m, "patch_embed.proj.bias", {D});
  for (int i = 0; i < c.depth; ++i) {
    const std::string b = "blocks." + std::to_string(i) + ".";
    add_param(m, b + "attn.in_proj_weight", {3 * D, D});
    add_param(m, b + "attn.in_proj_bias", {3 * D});
    add_param(m, b + "attn.out_proj.weight", {D, D});
    add_param(m, b + "attn.out_proj.bias", {D});
    add_param(m, b + "mlp.0.weight", {c.mlp_hidden, D});
    add_param(m, b + "mlp.0.bias", {c.mlp_hidden});
    add_param(m, b + "mlp.3.weight", {D, c.mlp_hidden});
    add_param(m, b + "mlp.3.bias", {D});
    add_param(m, b + "adaLN_modulation.1.weight", {6 * D, D});
    add_param(m, b + "adaLN_modulation.1.bias", {6 * D});
  }
  add_param(m, "final_layer.linear.weight", {m->dit->Nout, D});
  add_param(m, "final_layer.linear.bias", {m->dit->Nout});
  add_param(m, "final_layer.adaLN_modulation.1.weight", {2 * D, D});
  add_param(m, "final_layer.adaLN_modulation.1.bias", {2 * D});
}

void dit_build_params(cm_model *m) {
  const cm_dit_config &c = m->dit->cfg;
  const int64_t D = c.hidden_size, tx = D * c.time_multiple, p = c.patch_size, pt = c.t_patch_size;
  add_param(m, "spatial_pos_embed", {1, m->dit->Ns, D});
  add_param(m, "temporal_pos_embed", {1, c.t_max / pt, D});
  add_param(m, "dif_time_embeddings.time_blocks.0.weight", {TIME_ROWS, D});
  add_param(m, "dif_time_embeddings.time_blocks.1.weight", {tx, D});
  add_param(m, "dif_time_embeddings.time_blocks.1.bias", {tx});
  add_param(m, "dif_time_embeddings.time_blocks.3.weight", {tx, tx});
  add_param(m, "dif_time_embeddings.time_blocks.3.bias", {tx});
  add_param(m, "time_proj.0.weight", {D, tx});
  add_param(m, "time_proj.0.bias", {D});
  add_param(m, "patch_embed.proj.weight", {D, c.in_channels, pt, p, p});
  add_param(m, "patch_embed.proj.bias", {D});
  for (int i = 0; i < c.depth; ++i) {
    const std::string b = "blocks." + std::to_string(i) + ".";
    for (const char *attn : {"spatial_attn", "temporal_attn"}) {
      add_param(m, b + attn + ".in_proj_weight", {3 * D, D});
      add_param(m, b + attn + ".in_proj_bias", {3 * D});
      add_param(m, b + attn + ".out_proj.weight", {D, D});
      add_param(m, b + attn + ".out_proj.bias", {D});
    }
    add_param(m, b + "mlp.0.weight", {c.mlp_hidden, D});
    add_param(m, b + "mlp.0.bias", {c.mlp_hidden});
    add_param(m, b + "mlp.3.weight", {D, c.mlp_hidden});
    add_param(m, b + "mlp.3.bias", {D});
    add_param(m, b + "adaLN_modulation.1.weight", {9 * D, D});
    add_param(m, b + "adaLN_modulation.1.bias", {9 * D});
  }
  add_param(m, "final_layer.linear.weight", {m->dit->Nout, D});
  add_param(m, "final_layer.linear.bias", {m->dit->Nout});
  add_param(m, "final_layer.adaLN_modulation.1.weight", {2 * D, D});
  add_param(m, "final_layer.adaLN_modulation.1.bias", {2 * D});
}

cm::DitGemmArgs dit_gemm_args(int pro, int epi, long long M, int N, int K) {
  cm::DitGemmArgs a{};
  a.pro = pro; a.epi = epi; a.M = M; a.N = N; a.K = K;
  a.grp = (int)std::max(1LL, M); a.tok = 1;   // identity row map
  return a;
}

// Conditioning tables for all 1000 t (DiT4D_V4.py:363, 134-137, 216): e = time_blocks(t), c = SiLU(time_proj(e)); every
// adaLN_modulation applies SiLU(c) before its Linear.  The table row t holds each block's 9 chunks and the final layer's 2.
// DiT2D computes the same chain (DiT2D.py:275, 94-97, 117-119) with 6 chunks per block.  Runs again from cm_dit_train_sync, on
// the buffers of the first call.
int dit_build_tables(cm_model *m) {
  cm_dit_plan &d = *m->dit;
  const cm_dit_config &c = d.cfg;
  const int D = c.hidden_size, tx = D * c.time_multiple;
  if (!d.modtab) {
    if (dev_alloc(m, (void **)&d.modtab, (size_t)TIME_ROWS * d.ldmod * sizeof(float))) return 1;
    if (dev_alloc(m, (void **)&d.tab_h1, (size_t)TIME_ROWS * tx * sizeof(float))) return 1;
    if (dev_alloc(m, (void **)&d.tab_e, (size_t)TIME_ROWS * tx * sizeof(float))) return 1;
    if (dev_alloc(m, (void **)&d.tab_cs, (size_t)TIME_ROWS * D * sizeof(float))) return 1;
  }
  float *h1 = d.tab_h1, *e = d.tab_e, *cs = d.tab_cs;
  hipStream_t st = m->stream;
  cm::DitGemmArgs a = dit_gemm_args(cm::DIT_PRO_NONE, cm::DIT_EPI_SILU, TIME_ROWS, tx, D);
  a.A = d.w[2]; a.lda = D; a.W = d.w[3]; a.bias = d.w[4]; a.Y = h1; a.ldy = tx;
  CM_HIP(cm::launch_dit_gemm(a, st));
  a = dit_gemm_args(cm::DIT_PRO_NONE, cm::DIT_EPI_BIAS, TIME_ROWS, tx, tx);
  a.A = h1; a.lda = tx; a.W = d.w[5]; a.bias = d.w[6]; a.Y = e; a.ldy = tx;
  CM_HIP(cm::launch_dit_gemm(a, st));
  a = dit_gemm_args(cm::DIT_PRO_NONE, cm::DIT_EPI_SILU2, TIME_ROWS, D, tx);
  a.A = e; a.lda = tx; a.W = d.w[7]; a.bias = d.w[8]; a.Y = cs; a.ldy = D;
  CM_HIP(cm::launch_dit_gemm(a, st));
  const int nch = d.nchunk(), pb = d.per_block();
  for (int i = 0; i <= c.depth; ++i) {
    const bool fin = i == c.depth;
    const int wi = fin ? DIT_HEAD + pb * c.depth + 2 : DIT_HEAD + pb * i + pb - 2;
    a = dit_gemm_args(cm::DIT_PRO_NONE, cm::DIT_EPI_BIAS, TIME_ROWS, fin ? 2 * D : nch * D, D);
    a.A = cs; a.lda = D; a.W = d.w[wi]; a.bias = d.w[wi + 1]; a.Y = d.modtab + (size_t)i * nch * D; a.ldy = d.ldmod;
    CM_HIP(cm::launch_dit_gemm(a, st));
  }
  CM_HIP(hipStreamSynchronize(st));
  return 0;
}

int dit_finalize(cm_model *m) {
  DevGuard g(m->device);
  cm_dit_plan &d = *m->dit;
  const cm_dit_config &c = d.cfg;
  const size_t B = (size_t)c.max_batch, rows = B * d.tok, D = (size_t)c.hidden_size;
  const size_t vox = (size_t)m->L() * c.rows * c.cols * 8;
  if (dev_alloc(m, (void **)&m->tbuf, B * sizeof(long long))) return 1;
  CM_HIP(hipMemset(m->tbuf, 0xff, B * sizeof(long long)));   // -1: "no forward has written this sample" (dit_debug_activation)
  if (dev_alloc(m, (void **)&m->x8, B * vox * sizeof(float))) return 1;
  if (dev_alloc(m, (void **)&m->eps_cl, B * vox * sizeof(float))) return 1;
  CM_HIP(hipMemset(m->x8, 0, B * vox * sizeof(float)));
  CM_HIP(hipMemset(m->eps_cl, 0, B * vox * sizeof(float)));
  if (dev_alloc(m, (void **)&d.X, rows * D * sizeof(float))) return 1;
  if (dev_alloc(m, (void **)&d.QKV, rows * 3 * D * sizeof(float))) return 1;
  if (dev_alloc(m, (void **)&d.AO, rows * D * sizeof(float))) return 1;
  if (dev_alloc(m, (void **)&d.Hm, rows * (size_t)c.mlp_hidden * sizeof(float))) return 1;
  d.w.clear();
  for (const Param &p : m->params) {
    float *dp = nullptr;
    if (upload(m, p.host, &dp)) return 1;
    d.w.push_back(dp);
  }
  if (dit_build_tables(m)) return 1;
  if (m->precision == CM_PRECISION_F16 || m->precision == CM_PRECISION_F16A) {   // the fp32 copies stay: the tables above and cm_model_get_param read them
    d.w16.assign(d.w.size(), nullptr);
    std::vector<_Float16> h16;
    const int *wsel = d.full ? DIT2D_F16_W : DIT_F16_W;
    const int nsel = d.full ? 4 : 6;
    for (int i = 0; i < c.depth; ++i)
      for (int s = 0; s < nsel; ++s) {
        const int j = wsel[s];
        const size_t wi = (size_t)(DIT_HEAD + d.per_block() * i + j);
        const std::vector<float> &h = m->params[wi].host;
        h16.resize(h.size());
        for (size_t e = 0; e < h.size(); ++e) h16[e] = (_Float16)h[e];   // round-to-nearest-even, no clamp
        _Float16 *dp = nullptr;
        if (dev_alloc(m, (void **)&dp, h16.size() * sizeof(_Float16))) return 1;
        CM_HIP(hipMemcpy(dp, h16.data(), h16.size() * sizeof(_Float16), hipMemcpyHostToDevice));
        d.w16[wi] = dp;
      }
  }
  const size_t per = (size_t)m->per_sample();
  const size_t per_past = (size_t)c.in_channels * c.rows * c.cols * c.past_len;
  if (dev_alloc(m, (void **)&m->xstate, B * per * sizeof(float))) return 1;
  if (dev_alloc(m, (void **)&m->stage_fut, B * per * sizeof(float))) return 1;
  if (dev_alloc(m, (void **)&m->stage_out, B * per * sizeof(float))) return 1;
  if (dev_alloc(m, (void **)&m->stage_past, B * per_past * sizeof(float))) return 1;
  CM_HIP(hipDeviceSynchronize());
  m->finalized = true;
  return 0;
}

// One DiT4D_V4.forward (DiT4D_V4.py:347-375) for the B samples starting at b0: reads x8 and tbuf, writes eps_cl frames
// of the future slots.  Capturable: no allocation, synchronisation or host read; t comes from tbuf on the device.
// `nblocks`: stop after that many blocks (depth: the whole forward with the final layer; fewer: the residual stream X is
// left as that stage wrote it and eps_cl is untouched -- dit_debug_activation).
// f16 plan (d.w16 filled): the six token Linears of every block take dit_gemm_f16_kernel on the pre-rounded weights; the patch
// embedding, the final layer, LayerNorm + modulate, both attention kernels, the gates and every tensor stay fp32.
// f16a plan (a DiT2D handle with d.w16 filled): the four token Linears of every block likewise, and the full attention takes
// dit_attn_full_f16_kernel (both products on f16 operands, fp32 softmax); everything else as above.
int dit_forward(cm_model *m, int B, hipStream_t st, int b0, int nblocks) {
  const cm_dit_plan &d = *m->dit;
  const cm_dit_config &c = d.cfg;
  const int D = c.hidden_size, D3 = 3 * D, mlp = c.mlp_hidden, nq = d.Tp - d.qs;
  const long long r0 = (long long)b0 * d.tok, M = (long long)B * d.tok;
  const size_t vox = (size_t)m->L() * c.rows * c.cols * 8;
  float *X = d.X + r0 * D, *QKV = d.QKV + r0 * D3, *AO = d.AO + r0 * D, *Hm = d.Hm + r0 * mlp;
  cm::DitGemmArgs base{};
  base.tok = d.tok; base.tbuf = m->tbuf + b0; base.mod = d.modtab; base.ldmod = d.ldmod;
  base.L = m->L(); base.Hh = c.rows; base.Ww = c.cols; base.p = c.patch_size; base.pt = c.t_patch_size;
  base.Ns = d.Ns; base.wpn = c.cols / c.patch_size; base.Cout = c.out_channels;
  auto gemm = [&](int pro, int epi, long long rows, int N, int K) {
    cm::DitGemmArgs a = base;
    a.pro = pro; a.epi = epi; a.M = rows; a.N = N; a.K = K;
    a.grp = (int)rows;
    return a;
  };
  auto future_rows = [&](cm::DitGemmArgs &a, int slots) {   // logical row -> token row of slot >= qs
    a.M = (long long)B * slots * d.Ns; a.grp = slots * d.Ns; a.grp_stride = d.tok; a.grp_off = d.qs * d.Ns;
  };
  // patch embedding + position embeddings (DiT4D_V4.py:365-367)
  cm::DitGemmArgs a = gemm(cm::DIT_PRO_PATCH, cm::DIT_EPI_PATCH, M, D, d.Kp);
  a.x8 = m->x8 + (size_t)b0 * vox; a.W = d.w[9]; a.bias = d.w[10]; a.Y = X; a.ldy = D; a.spos = d.w[0]; a.tpos = d.w[1];
  CM_HIP(cm::launch_dit_gemm(a, st));
  cm::DitAttnArgs at{QKV, AO, B, d.Tp, d.Ns, d.qs, D, c.num_heads};
  const int nch = d.nchunk(), pb = d.per_block();
  const bool f16 = !d.w16.empty();
  for (int i = 0; i < nblocks; ++i) {
    const float *const *w = d.w.data() + DIT_HEAD + pb * i;
    const int mo = i * nch * D;
    auto launch = [&](cm::DitGemmArgs &g, int j) {   // the token Linear on the block's weight j, in the plan's form
      g.W = w[j]; g.bias = w[j + 1];
      if (f16) { g.f16 = 1; g.Wh = d.w16[DIT_HEAD + pb * i + j]; }
      return cm::launch_dit_gemm(g, st);
    };
    if (d.full) {
      // self-attention over all tokens of the sample, gated residual on every row (DiT2D.py:104-106)
      a = gemm(cm::DIT_PRO_LN, cm::DIT_EPI_BIAS, M, D3, D);
      a.A = X; a.lda = D; a.Y = QKV; a.ldy = D3; a.off_shift = mo; a.off_scale = mo + D;
      CM_HIP(launch(a, 0));
      CM_HIP(d.attn16() ? cm::launch_dit_attn_full_f16(at, st) : cm::launch_dit_attn_full(at, st));
      a = gemm(cm::DIT_PRO_NONE, cm::DIT_EPI_GATE, M, D, D);
      a.A = AO; a.lda = D; a.Y = X; a.ldy = D; a.off_gate = mo + 2 * D;
      CM_HIP(launch(a, 2));
      // MLP (:107-108)
      a = gemm(cm::DIT_PRO_LN, cm::DIT_EPI_GELU, M, mlp, D);
      a.A = X; a.lda = D; a.Y = Hm; a.ldy = mlp; a.off_shift = mo + 3 * D; a.off_scale = mo + 4 * D;
      CM_HIP(launch(a, 4));
      a = gemm(cm::DIT_PRO_NONE, cm::DIT_EPI_GATE, M, D, mlp);
      a.A = Hm; a.lda = mlp; a.Y = X; a.ldy = D; a.off_gate = mo + 5 * D;
      CM_HIP(launch(a, 6));
      continue;
    }
    // spatial self-attention (DiT4D_V4.py:160-169)
    a = gemm(cm::DIT_PRO_LN, cm::DIT_EPI_BIAS, M, D3, D);
    a.A = X; a.lda = D; a.Y = QKV; a.ldy = D3; a.off_shift = mo; a.off_scale = mo + D;
    CM_HIP(launch(a, 0));
    CM_HIP(cm::launch_dit_attn_spatial(at, st));
    a = gemm(cm::DIT_PRO_NONE, cm::DIT_EPI_GATE, M, D, D);
    a.A = AO; a.lda = D; a.Y = X; a.ldy = D; a.off_gate = mo + 2 * D;
    CM_HIP(launch(a, 2));
    // temporal cross-attention: keys / values over all slots, queries and the residual update on slots >= qs (:173-198)
    a = gemm(cm::DIT_PRO_LN, cm::DIT_EPI_BIAS, M, D3, D);
    a.A = X; a.lda = D; a.Y = QKV; a.ldy = D3; a.off_shift = mo + 3 * D; a.off_scale = mo + 4 * D;
    CM_HIP(launch(a, 4));
    CM_HIP(cm::launch_dit_attn_temporal(at, st));
    a = gemm(cm::DIT_PRO_NONE, cm::DIT_EPI_GATE, M, D, D);
    future_rows(a, nq);
    a.a_compact = 1; a.A = AO; a.lda = D; a.Y = X; a.ldy = D; a.off_gate = mo + 5 * D;
    CM_HIP(launch(a, 6));
    // MLP (:201-202)
    a = gemm(cm::DIT_PRO_LN, cm::DIT_EPI_GELU, M, mlp, D);
    a.A = X; a.lda = D; a.Y = Hm; a.ldy = mlp; a.off_shift = mo + 6 * D; a.off_scale = mo + 7 * D;
    CM_HIP(launch(a, 8));
    a = gemm(cm::DIT_PRO_NONE, cm::DIT_EPI_GATE, M, D, mlp);
    a.A = Hm; a.lda = mlp; a.Y = X; a.ldy = D; a.off_gate = mo + 8 * D;
    CM_HIP(launch(a, 10));
  }
  if (nblocks < c.depth) return 0;
  // final layer + unpatchify, future slots only: slots < qs hold past frames only (:223-225, :93-99; DiT2D computes
  // every frame and slices, DiT2D.py:292-296 -- rows are independent)
  const float *const *wf = d.w.data() + DIT_HEAD + pb * c.depth;
  a = gemm(cm::DIT_PRO_LN, cm::DIT_EPI_UNPATCH, M, d.Nout, D);
  future_rows(a, nq);
  a.A = X; a.lda = D; a.W = wf[0]; a.bias = wf[1]; a.Y = m->eps_cl + (size_t)b0 * vox;
  a.off_shift = c.depth * nch * D; a.off_scale = c.depth * nch * D + D;
  CM_HIP(cm::launch_dit_gemm(a, st));
  return 0;
}

// Algorithmic FLOPs of one forward (2 per multiply-add; the final layer on the future slots it runs on) and the bytes
// of the weights plus the sampler tensors it reads and writes.
int dit_cost(const cm_model *m, int B, double *flops, double *bytes) {
  const cm_dit_plan &d = *m->dit;
  const cm_dit_config &c = d.cfg;
  const double D = c.hidden_size, mlp = c.mlp_hidden, tok = d.tok, Ns = d.Ns, Tp = d.Tp, nq = d.Tp - d.qs;
  double f = 2.0 * tok * d.Kp * D;
  const double blk = d.full
                   ? 2.0 * tok * D * 3.0 * D                    // packed q|k|v projection
                     + 4.0 * tok * tok * D                      // q k^T and P V over all S = tok keys
                     + 2.0 * tok * D * D                        // out-projection
                     + 2.0 * (2.0 * tok * D * mlp)              // MLP
                   : 2.0 * (2.0 * tok * D * 3.0 * D)          // two packed q|k|v projections
                     + 4.0 * Tp * Ns * Ns * D                   // spatial q k^T and P V
                     + 2.0 * tok * D * D                        // spatial out-projection
                     + 4.0 * Ns * nq * Tp * D                   // temporal q k^T and P V
                     + 2.0 * nq * Ns * D * D                    // temporal out-projection (future slots)
                     + 2.0 * (2.0 * tok * D * mlp);             // MLP
  f += c.depth * blk + 2.0 * nq * Ns * D * d.Nout;
  double wb = 0;
  for (const Param &p : m->params) wb += 4.0 * p.numel();
  if (flops) *flops = f * B;
  if (bytes) *bytes = wb + 4.0 * B * 2.0 * (double)m->L() * c.rows * c.cols * 8;
  return 0;
}

// `le`: what a cm_sample_loop step leaves out at the ends of the UNet (LoopEnds; null: the whole forward)
int denoise(cm_model *m, const FwdPlan &plan, hipStream_t st, int b0, int slab, const LoopEnds *le = nullptr) {
  return m->dit ? dit_forward(m, plan.ctx.B, st, b0, m->dit->cfg.depth) : run_ops(m, plan, st, b0, slab, le);
}

// cm_debug_activation of a DiT handle: "patch_embed" or "blocks.<i>" -> the residual stream [B][T_p * N_s][D] after that
// stage, as a forward hook on the reference module sees it.  x8 and tbuf still hold the last forward's inputs, so the
// forward is run again from them, stopped after the stage, and X copied out; B is the number of leading samples whose t a
// forward has written (dit_finalize leaves -1; samples past the last batch are those of an earlier, larger one).
int dit_debug_activation(cm_model *m, const char *name, float *h_out, int64_t capacity, int64_t shape[5]) {
  const cm_dit_plan &d = *m->dit;
  const cm_dit_config &c = d.cfg;
  int nblocks = -1;
  if (!std::strcmp(name, "patch_embed")) {
    nblocks = 0;
  } else if (!std::strncmp(name, "blocks.", 7) && name[7] >= '0' && name[7] <= '9') {
    char *end = nullptr;
    const long i = std::strtol(name + 7, &end, 10);
    if (!*end && i >= 0 && i < c.depth) nblocks = (int)i + 1;
  }
  if (nblocks < 0) return fail("no DiT activation named %s (patch_embed, blocks.0 .. blocks.%d)", name, c.depth - 1);
  DevGuard g(m->device);
  CM_HIP(hipDeviceSynchronize());
  std::vector<long long> t((size_t)c.max_batch);
  CM_HIP(hipMemcpy(t.data(), m->tbuf, t.size() * sizeof(long long), hipMemcpyDeviceToHost));
  int B = 0;
  while (B < c.max_batch && t[B] >= 0 && t[B] < TIME_ROWS) ++B;
  if (B == 0) return fail("cm_debug_activation: no forward has run on this DiT handle");
  const int64_t n = (int64_t)B * d.tok * c.hidden_size;
  if (capacity < n) return fail("capacity %lld < %lld", (long long)capacity, (long long)n);
  if (dit_forward(m, B, m->stream, 0, nblocks)) return 1;
  CM_HIP(hipStreamSynchronize(m->stream));
  CM_HIP(hipMemcpy(h_out, d.X, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
  if (shape) { shape[0] = B; shape[1] = d.tok; shape[2] = c.hidden_size; shape[3] = 1; shape[4] = 1; }
  return 0;
}

// cm_debug_dit_attn: one launch of the full-attention kernel of the handle's plan on the caller's q|k|v, through the handle's own
// QKV / AO workspace (a later forward overwrites both before it reads them).
int dit_debug_attn(cm_model *m, const float *h_qkv, float *h_out, int B) {
  const cm_dit_plan &d = *m->dit;
  const cm_dit_config &c = d.cfg;
  if (B < 1 || B > c.max_batch) return fail("cm_debug_dit_attn: B = %d is outside [1, max_batch = %d]", B, c.max_batch);
  DevGuard g(m->device);
  const size_t n = (size_t)B * d.tok * c.hidden_size;
  CM_HIP(hipDeviceSynchronize());
  CM_HIP(hipMemcpy(d.QKV, h_qkv, 3 * n * sizeof(float), hipMemcpyHostToDevice));
  const cm::DitAttnArgs at{d.QKV, d.AO, B, d.Tp, d.Ns, d.qs, c.hidden_size, c.num_heads};
  CM_HIP(d.attn16() ? cm::launch_dit_attn_full_f16(at, m->stream) : cm::launch_dit_attn_full(at, m->stream));
  CM_HIP(hipStreamSynchronize(m->stream));
  CM_HIP(hipMemcpy(h_out, d.AO, n * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}

// The handle of an admitted configuration (the callers have checked it); `full`: the DiT2D variant.
int dit_make_handle(const cm_dit_config &c, bool full, cm_model **out) {
  if (c.device >= 0) {
    int ndev = 0;
    CM_HIP(hipGetDeviceCount(&ndev));
    if (c.device >= ndev) return fail("device %d not available (%d devices)", c.device, ndev);
  }
  const int Ns = (c.rows / c.patch_size) * (c.cols / c.patch_size), Tp = (c.past_len + c.future_len) / c.t_patch_size;
  auto m = std::make_unique<cm_model>();
  m->cfg.in_channels = c.in_channels; m->cfg.out_channels = c.out_channels;
  m->cfg.rows = c.rows; m->cfg.cols = c.cols; m->cfg.past_len = c.past_len; m->cfg.future_len = c.future_len;
  m->cfg.time_multiple = c.time_multiple; m->cfg.max_batch = c.max_batch; m->cfg.device = c.device;
  m->device = c.device;
  m->dit = new cm_dit_plan;
  cm_dit_plan &d = *m->dit;
  d.cfg = c;
  d.full = full;
  d.Ns = Ns; d.Tp = Tp; d.qs = c.past_len / c.t_patch_size; d.tok = Tp * Ns;
  d.Kp = c.in_channels * c.t_patch_size * c.patch_size * c.patch_size;
  d.Nout = c.t_patch_size * c.out_channels * c.patch_size * c.patch_size;
  d.ldmod = c.depth * d.nchunk() * c.hidden_size + 2 * c.hidden_size;
  if (full) dit2d_build_params(m.get()); else dit_build_params(m.get());
  if (m->device >= 0) {
    DevGuard g(m->device);
    CM_HIP(hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking));
    for (int i = 1; i < 4; ++i) {
      CM_HIP(hipStreamCreateWithFlags(&m->lane_stream[i], hipStreamNonBlocking));
      CM_HIP(hipEventCreateWithFlags(&m->ev_join[i], hipEventDisableTiming));
    }
    CM_HIP(hipEventCreateWithFlags(&m->ev_fork, hipEventDisableTiming));
  }
  *out = m.release();
  return 0;
}

}  // namespace

extern "C" int cm_model_create_dit2d(const cm_dit2d_config *cfg, cm_model **out) {
  if (!cfg || !out) return fail("null argument");
  const cm_dit2d_config &c = *cfg;
  if (c.in_channels < 1 || c.in_channels > 8 || c.out_channels < 1 || c.out_channels > 8) return fail("in/out channels must be in [1,8]");
  if (c.max_batch < 1) return fail("max_batch must be >= 1");
  if (c.depth < 1 || c.time_multiple < 1 || c.past_len < 1 || c.future_len < 1) return fail("depth, time_multiple, past_len and future_len must be >= 1");
  if (c.patch_size < 1) return fail("patch_size must be >= 1");
  if (c.rows < 1 || c.cols < 1 || c.rows % c.patch_size || c.cols % c.patch_size)
    return fail("grid %dx%d is not divisible by patch_size %d (DiT2D.py:17-20)", c.rows, c.cols, c.patch_size);
  const int L = c.past_len + c.future_len;
  if (L > c.t_max) return fail("past_len + future_len = %d frames exceed the t_max = %d rows of temporal_pos_embed (DiT2D.py:244)", L, c.t_max);
  if (c.num_heads < 1 || c.hidden_size < 1 || c.hidden_size % c.num_heads)
    return fail("hidden_size %d is not divisible by num_heads %d", c.hidden_size, c.num_heads);
  if (c.hidden_size / c.num_heads != 64) return fail("head dim %d: the DiT attention kernels are built for head dim 64", c.hidden_size / c.num_heads);
  if (c.mlp_hidden < 64 || c.mlp_hidden % 64) return fail("mlp_hidden %d must be a positive multiple of 64", c.mlp_hidden);
  const long long S = (long long)L * (c.rows / c.patch_size) * (c.cols / c.patch_size);
  if (S > 1024) return fail("%lld tokens per sample ((past_len + future_len) * patches): the DiT2D plan admits at most 1024", S);
  cm_dit_config v{};
  v.in_channels = c.in_channels; v.out_channels = c.out_channels; v.rows = c.rows; v.cols = c.cols;
  v.past_len = c.past_len; v.future_len = c.future_len; v.patch_size = c.patch_size; v.t_patch_size = 1;
  v.hidden_size = c.hidden_size; v.depth = c.depth; v.num_heads = c.num_heads; v.mlp_hidden = c.mlp_hidden;
  v.time_multiple = c.time_multiple; v.t_max = c.t_max; v.max_batch = c.max_batch; v.device = c.device;
  return dit_make_handle(v, true, out);
}

extern "C" int cm_model_create_dit(const cm_dit_config *cfg, cm_model **out) {
  if (!cfg || !out) return fail("null argument");
  const cm_dit_config &c = *cfg;
  if (c.in_channels < 1 || c.in_channels > 8 || c.out_channels < 1 || c.out_channels > 8) return fail("in/out channels must be in [1,8]");
  if (c.max_batch < 1) return fail("max_batch must be >= 1");
  if (c.depth < 1 || c.time_multiple < 1 || c.past_len < 1 || c.future_len < 1) return fail("depth, time_multiple, past_len and future_len must be >= 1");
  if (c.patch_size < 1 || c.t_patch_size < 1) return fail("patch_size and t_patch_size must be >= 1");
  if (c.rows < 1 || c.cols < 1 || c.rows % c.patch_size || c.cols % c.patch_size)
    return fail("grid %dx%d is not divisible by patch_size %d (DiT4D_V4.py:25-28)", c.rows, c.cols, c.patch_size);
  const int L = c.past_len + c.future_len;
  if (L % c.t_patch_size) return fail("past_len + future_len = %d is not divisible by t_patch_size %d (DiT4D_V4.py:257)", L, c.t_patch_size);
  const int Tp = L / c.t_patch_size, tslots = c.t_max / c.t_patch_size;
  if (Tp > tslots) return fail("T_p = %d temporal slots exceed the %d rows of temporal_pos_embed (t_max %d / t_patch_size %d)", Tp, tslots, c.t_max, c.t_patch_size);
  if (c.num_heads < 1 || c.hidden_size < 1 || c.hidden_size % c.num_heads)
    return fail("hidden_size %d is not divisible by num_heads %d", c.hidden_size, c.num_heads);
  if (c.hidden_size / c.num_heads != 64) return fail("head dim %d: the DiT attention kernels are built for head dim 64", c.hidden_size / c.num_heads);
  if (c.mlp_hidden < 64 || c.mlp_hidden % 64) return fail("mlp_hidden %d must be a positive multiple of 64", c.mlp_hidden);
  const int Ns = (c.rows / c.patch_size) * (c.cols / c.patch_size);
  if (Ns > 64) return fail("%d spatial patches: the spatial attention kernel holds at most 64", Ns);
  if (Tp > 8) return fail("%d temporal slots: the temporal attention kernel holds at most 8", Tp);
  if (c.past_len / c.t_patch_size >= Tp) return fail("no future temporal slot: past_len / t_patch_size = %d of %d", c.past_len / c.t_patch_size, Tp);
  return dit_make_handle(c, false, out);
}
