// Training step host orchestration (included at the end of cm_model.cpp: same translation
// unit, shares its internal types).  Mirrors DDPM_model._train_step + optimizer.step()
// (/root/reference/models/diffusion/ddpm.py:111-121,142-144): q-sample, UNet forward with
// Dropout3d, MSE, full backward, Adam with coupled L2.
//
// The backward walks the forward op list in reverse.  For a conv op
//   out = conv(T(in0|in1)) + temb + resid,   T = pm * silu(groupnorm(.)) or identity
// it accumulates  d resid += dY,  d temb_proj = sum_v dY,  d bias = sum dY,
// dW = wgrad(dY, T(in)) on the matrix cores, and the data gradient
// dA = conv(dY, W flipped/transposed) through the forward conv kernel, followed by the
// GroupNorm/SiLU backward kernels (or a plain accumulate when T is the identity).
// Stride-2 convs take the zero-stuffed dY, upsample convs go through the materialised
// upsampled tensor (wgrad) and a 2x2x2 sum-pool (dgrad).
//
// Autocast (cm_train_set_autocast; the reference wraps this step in torch.amp.autocast, ddpm.py:116-120): the layers on the
// Winograd route run forward, data gradient and weight gradient on f16 operands with fp32 accumulation (the f16 form of the
// forward kernel, wgrad_wino_f16_kernel), the loss gradient is multiplied by 2^k and the flat gradient buffer by 2^-k at the
// end of the pass; everything else, and every launch of a handle that never switches it on, is unchanged.

struct cm_train_state {
  std::set<const Act *> gset;  // backward pass: tensors whose gradient buffer has received a contribution
  // master weights, gradients, Adam moments; frozen: the sinusoid table, first tensor of the state_dict (requires_grad False, embeddings.py:24)
  OptStore opt;
  float dropout = 0.1f;  // nn.Dropout3d(p) of the ResnetBlocks (layers.py:42), cfg DROPOUT_RATE
  hipEvent_t ev_dy = nullptr, ev_wdone = nullptr;   // backward: weight-gradient launches run on a second stream (see backward_ops)
  // derived device tensors refreshed from the master weights (opt.p) after every optimizer step
  struct Derived { float *dst; int *d_idx; int nk; long long n; bool bwd_only; };
  std::vector<Derived> derived;
  cm::PackJob *d_jobs = nullptr;   // the same list as one device-side job table
  int *d_blk2job = nullptr; long long pack_blocks = 0;   // workgroup -> job (each job owns whole workgroups)
  // Winograd-transformed weight tensors: structured re-derivation (27 indices per (co, ci) pair)
  struct DerivedWino { float *dst; int *d_idx27; int Co, Ci, Ci_pad; long long n; };
  std::vector<DerivedWino> derived_wino;
  cm::WinoPackJob *d_wjobs = nullptr; int *d_wblk2job = nullptr; long long wpack_blocks = 0;
  cm::WinoPackJob *d_wjobs16 = nullptr;   // autocast: the same jobs writing the f16 fragments (wino_pack_jobs_f16_kernel; same workgroup map)
  int njobs = 0;
  long long pack_total = 0;
  // per conv op: data-gradient launch
  struct Dgrad {
    bool have = false;
    cm::ConvArgs ca{};
    int MB = 1, NB = 1;
    int *d_hv = nullptr, *d_mt = nullptr;
    float *wfrag = nullptr, *zero_bias = nullptr;
    bool wino = false;          // stride-1 3x3x3 data gradient on an even in-plane grid: Winograd kernel (cm_conv_wino.hip)
    float *wwino = nullptr;
    float *wwino_b6 = nullptr;  // six-term bf16 split of wwino (pack_wino_b6 order), re-derived after every optimizer step
    long long wwino_floats = 0;
    float *wwino16 = nullptr;   // autocast: f16 sibling of wwino_b6 (pack_wino_f16 order), allocated when mode 1 is first set
    // two-plane grids: the data gradient on the whole-sample kernel conv_qr2 in its six-term form (no normalisation: `raw`)
    bool qr = false;
    float *wqr = nullptr, *wqr_b6 = nullptr;
    long long wqr_floats = 0;
    bool wwg = false;           // weight gradient in the Winograd domain (the forward op is a Winograd layer)
    cm::ConvArgs wwa{};
    // weight-gradient geometry when it differs from the forward op (parity / upsample convs)
    bool own_wgeom = false;
    cm::ConvArgs wa{};
    int wMB = 1;
    int *w_hv = nullptr, *w_mt = nullptr;
  };
  std::vector<Dgrad> dg;  // indexed like m->ops
  // scratch
  float *scrA = nullptr, *scrB = nullptr, *scrC = nullptr;  // [B][Vfull][Cmax]
  float *wpart = nullptr; size_t wpart_floats = 0;
  float *tmp_bc = nullptr;       // [B][Cmax]
  cm::CopyJob *d_cp_jobs = nullptr; int n_cp_jobs = 0; long long cp_max = 0;
  float *attn_big = nullptr; size_t attn_big_floats = 0;   // S x S scratch of the attention backward at large token counts
  // deferred batch reductions: every conv / GroupNorm of the backward pass leaves its per-sample sums in its own region
  // of bs_pool; one job-table launch at the end turns them into the parameter gradients (the table is recorded during
  // the first pass: the op sequence, region offsets and strides never change, only B, which is a launch argument)
  float *bs_pool = nullptr; size_t bs_pool_floats = 0, bs_cursor = 0;
  std::vector<cm::BsumJob> bs_jobs; cm::BsumJob *d_bs_jobs = nullptr; bool bs_ready = false; int bs_maxC = 0;
  std::vector<cm::VsumJob> vs_jobs; cm::VsumJob *d_vs_jobs = nullptr; int vs_maxC = 0;   // the per-sample voxel sums feeding them, deferred the same way
  float *vs_part = nullptr;      // [16][B][Cmax] voxel-slice partials of the bias / time-row gradient sums
  float *dproj = nullptr;        // [B][nproj]
  float *train_temb = nullptr;   // [B][nproj] forward projection of the batch's timesteps
  long long *iota = nullptr;     // [B] 0,1,2,...
  float *gnb_part = nullptr, *gnb_coef = nullptr, *gnb_dgb = nullptr;
  float *time_ws = nullptr, *dWd_all = nullptr, *dbd_all = nullptr;
  float *xt = nullptr, *pred = nullptr, *eps_dev = nullptr;
  long long draws = 0;
  long long sample_base = 0;     // global index of this rank's sample 0 (data-parallel training)
  int Cmax = 0;
  // autocast (cm_train_set_autocast): f16 operands in the Winograd layers' three passes, loss gradient scaled by 2^ls_k
  int autocast = 0, ls_req = -1;   // mode; requested scale exponent (< 0: automatic)
  int ls_k = 0;                    // exponent of the step in flight (0 in fp32 mode: scale 1, no unscale launch)
  int ls_last_B = 0;               // batch of the last autocast step (cm_train_get_autocast)
  bool ac_ready = false;           // the f16 fragments (Op::d_wwino16t, Dgrad::wwino16) exist
};

void cm_free_train_state(cm_train_state *t) {
  if (t) {
    if (t->ev_dy) hipEventDestroy(t->ev_dy);
    if (t->ev_wdone) hipEventDestroy(t->ev_wdone);
  }
  delete t;
}

namespace {

size_t off_of(cm_model *m, const std::string &name) { return m->train->opt.off[m->pindex.at(name)]; }   // offset in the flat buffers
float *grad_of(cm_model *m, const std::string &name) { return m->train->opt.g + off_of(m, name); }

// positions in the flat parameter buffer (opt.p) of a tensor's elements, in state_dict order
std::vector<int> flat_index(cm_model *m, const std::string &name) {
  std::vector<int> v((size_t)P(m, name).numel());
  std::iota(v.begin(), v.end(), (int)off_of(m, name));
  return v;
}
// ... of a conv weight's elements, in the internal tap order [Co][Ci][t]: the layouts of cm_pack.h, fed with these instead of the
// values, give the index maps of the device re-pack
std::vector<int> ref_index_internal(cm_model *m, const std::string &wname, int Co, int Ci, int ntaps) {
  return to_internal_taps(flat_index(m, wname).data(), Co, Ci, ntaps);
}

// a device tensor re-derived from opt.p after every optimizer step: element i = sum over its nk indices (-1: none) of opt.p[index]
int add_derived(cm_model *m, float *dst, const int *idx, size_t count, int nk, bool bwd_only = false) {
  cm_train_state::Derived d;
  d.dst = dst; d.nk = nk; d.n = (long long)(count / nk); d.bwd_only = bwd_only;
  if (dev_alloc(m, (void **)&d.d_idx, count * sizeof(int))) return 1;
  CM_HIP(hipMemcpy(d.d_idx, idx, count * sizeof(int), hipMemcpyHostToDevice));
  m->train->derived.push_back(d);
  return 0;
}
int add_derived(cm_model *m, float *dst, const std::vector<int> &idx, int nk, bool bwd_only = false) {
  return add_derived(m, dst, idx.data(), idx.size(), nk, bwd_only);
}
int add_derived(cm_model *m, float *dst, const std::vector<Src8> &idx) { return add_derived(m, dst, idx[0].data(), idx.size() * 8, 8); }

int add_derived_wino(cm_model *m, float *dst, const std::vector<int> &idx27, int Co, int Ci, int Ci_pad) {
  cm_train_state::DerivedWino d;
  d.dst = dst; d.Co = Co; d.Ci = Ci; d.Ci_pad = Ci_pad;
  d.n = (long long)((Co + 31) / 32) * 32 * Ci_pad * 3;   // threads: (padded co, padded ci, z tap)
  if ((long long)idx27.size() != (long long)Co * Ci * 27) return fail("Winograd weight map: %zu indices for %d x %d x 27", idx27.size(), Co, Ci);
  if (dev_alloc(m, (void **)&d.d_idx27, idx27.size() * sizeof(int))) return 1;
  CM_HIP(hipMemcpy(d.d_idx27, idx27.data(), idx27.size() * sizeof(int), hipMemcpyHostToDevice));
  m->train->derived_wino.push_back(d);
  return 0;
}

int tune_launch(cm_model *m, cm::ConvArgs &ca, int &MB, int NB, int *&d_hv, int *&d_mt, bool wgrad) {
  Op tmp;
  tmp.kind = OP_CONV; tmp.ca = ca; tmp.NB = NB;
  static Act dummy;
  tmp.stat_act = wgrad ? &dummy : nullptr;  // the weight-gradient kernel wants one sample per tile
  if (wgrad) tmp.ca.CK = 32;                 // ... and stages 32-channel rows whatever the forward chunking
  pick_tile(tmp, TUNE_BATCH);
  const int ck = ca.CK;
  ca = tmp.ca; ca.CK = ck; MB = tmp.MB;
  std::vector<int> hv((size_t)cm::conv_halo_voxels(ca)), mt((size_t)32 * MB);
  cm::conv_build_tables(ca, MB, hv.data(), mt.data());
  if (dev_alloc(m, (void **)&d_hv, hv.size() * sizeof(int))) return 1;
  if (dev_alloc(m, (void **)&d_mt, mt.size() * sizeof(int))) return 1;
  CM_HIP(hipMemcpy(d_hv, hv.data(), hv.size() * sizeof(int), hipMemcpyHostToDevice));
  CM_HIP(hipMemcpy(d_mt, mt.data(), mt.size() * sizeof(int), hipMemcpyHostToDevice));
  ca.hvtab = d_hv; ca.mtab = d_mt;
  return 0;
}

// The h2 fragments (f16 two-way splits of w * 2^k, cm_model.cpp: add_conv) re-derived from the MASTER weights of a handle that has
// trained: per layer, the weight and the GroupNorm affine of its input come back from the device (a few MB), the static range bound is
// checked again (a layer that no longer satisfies it keeps the six-term form: Op::h2_off), the fragments are packed on the host by the
// load-time code and copied over the existing buffers.  Called by the inference entry points when an optimizer step (or a parameter
// load into the training state) has left the fragments behind: once per train -> sample transition, tens of milliseconds.
int refresh_h2(cm_model *m) {
  if (!m->h2_stale) return 0;
  cm_train_state *T = m->train;
  if (!T || m->precision != CM_PRECISION_F32) { m->h2_stale = false; return 0; }
  DevGuard g(m->device);
  CM_HIP(hipDeviceSynchronize());                   // the optimizer step's writes (any stream of this handle) have landed
  auto fetch = [&](const std::string &name, std::vector<float> *out) -> int {
    const Param &pr = P(m, name);
    out->resize((size_t)pr.numel());
    CM_HIP(hipMemcpy(out->data(), T->opt.p + off_of(m, name), out->size() * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
  };
  std::vector<float> w, gam, bet, frag;
  for (Op &op : m->ops) {
    if (op.kind == OP_ATTNBLK && op.d_win_h2 && op.d_wout_h2) {   // the whole-sample attention kernel's two weights
      std::vector<float> wo, fi, fo;
      if (fetch(op.win_name, &w) || fetch(op.wout_name, &wo)) return 1;
      attn_pack_h2(w.data(), wo.data(), op.E, &fi, &fo, &op.ab_in_oscale, &op.ab_out_oscale);
      CM_HIP(hipMemcpy(op.d_win_h2, fi.data(), fi.size() * sizeof(float), hipMemcpyHostToDevice));
      CM_HIP(hipMemcpy(op.d_wout_h2, fo.data(), fo.size() * sizeof(float), hipMemcpyHostToDevice));
      continue;
    }
    if (op.kind != OP_CONV || !(op.d_wwino_h2 || op.d_wqr_h2 || op.d_wfin_h2 || op.d_wups_h2)) continue;
    if (fetch(op.wname, &w)) return 1;
    op.h2_off = false;
    if (!op.d_wups_h2) {                             // (the upsample conv takes its range from the data, not from a GroupNorm bound)
      if (op.gn_op < 0) { op.h2_off = true; continue; }
      const Op &gop = m->ops[op.gn_op];
      if (fetch(gop.gname, &gam) || fetch(gop.bename, &bet)) return 1;
      if (!h2_bound_ok(gam, bet, gop, op.d_wwino_h2 ? 4.0 : 1.0)) { op.h2_off = true; continue; }
    }
    const H2Kind kind = op.d_wfin_h2 ? H2_FIN : op.d_wwino_h2 ? H2_WINO : op.d_wqr_h2 ? H2_QR : H2_UPS;
    float *dst = kind == H2_WINO ? op.d_wwino_h2 : kind == H2_QR ? op.d_wqr_h2 : op.d_wups_h2;
    const float ws = h2_pack(op, kind, w.data(), &frag);
    if (!(ws > 0.f)) { op.h2_off = true; continue; }
    if (kind == H2_FIN) CM_HIP(cm::launch_fin_pack(T->opt.p + off_of(m, op.wname), op.d_wfin_h2, op.ca.Co, 2, m->stream, ws));
    else CM_HIP(hipMemcpy(dst, frag.data(), frag.size() * sizeof(float), hipMemcpyHostToDevice));
    op.h2_oscale = 1.f / ws;
  }
  CM_HIP(hipStreamSynchronize(m->stream));
  m->h2_stale = false;
  return 0;
}

// autocast: the f16 fragments of the Winograd layers' forward and data gradient from the master weights, one job-table launch
int repack_f16(cm_model *m, hipStream_t st) {
  cm_train_state *T = m->train;
  if (!T->ac_ready) return 0;
  CM_HIP(cm::launch_wino_pack_jobs_f16(T->opt.p, T->d_wjobs16, T->d_wblk2job, T->wpack_blocks, st));
  return 0;
}

// the loss-scale exponent of a step at batch B: the requested one, or the largest k with 2^k <= B*C*H*W*F (loss gradient O(1))
int autocast_scale_log2(const cm_model *m, int B) {
  const cm_train_state *T = m->train;
  if (T->ls_req >= 0) return T->ls_req;
  const cm_unet_config &c = m->cfg;
  const long long N = (long long)B * c.out_channels * c.rows * c.cols * c.future_len;
  int k = 0;
  while (k < 24 && (2LL << k) <= N) ++k;
  return k;
}

int repack_all(cm_model *m, hipStream_t st) {
  cm_train_state *T = m->train;
  m->h2_stale = true;                               // (the h2 fragments follow lazily: refresh_h2)
  if (!T->d_jobs) {
    std::vector<cm::PackJob> jobs;
    std::vector<int> b2j;
    long long total = 0;
    for (auto &d : T->derived) {
      cm::PackJob j{};
      j.dst = d.dst; j.idx = d.d_idx; j.coef = nullptr; j.start = total; j.nk = d.nk;
      j.n = d.n; j.blk0 = (long long)b2j.size();
      for (long long k = 0; k < (d.n + 255) / 256; ++k) b2j.push_back((int)jobs.size());
      jobs.push_back(j);
      total += d.n;
    }
    if (dev_alloc(m, (void **)&T->d_jobs, jobs.size() * sizeof(cm::PackJob))) return 1;
    if (dev_alloc(m, (void **)&T->d_blk2job, b2j.size() * sizeof(int))) return 1;
    CM_HIP(hipMemcpy(T->d_jobs, jobs.data(), jobs.size() * sizeof(cm::PackJob), hipMemcpyHostToDevice));
    CM_HIP(hipMemcpy(T->d_blk2job, b2j.data(), b2j.size() * sizeof(int), hipMemcpyHostToDevice));
    T->njobs = (int)jobs.size();
    T->pack_total = total;
    T->pack_blocks = (long long)b2j.size();
  }
  CM_HIP(cm::launch_gather_pack_jobs(T->opt.p, T->d_jobs, T->d_blk2job, T->pack_blocks, st));
  if (!T->d_wjobs && !T->derived_wino.empty()) {
    std::vector<cm::WinoPackJob> jobs;
    std::vector<int> b2j;
    for (auto &d : T->derived_wino) {
      cm::WinoPackJob j{};
      j.dst = d.dst; j.idx27 = d.d_idx27; j.Co = d.Co; j.Ci = d.Ci; j.Ci_pad = d.Ci_pad; j.n = d.n; j.blk0 = (long long)b2j.size();
      for (long long k = 0; k < (d.n + 255) / 256; ++k) b2j.push_back((int)jobs.size());
      jobs.push_back(j);
    }
    if (dev_alloc(m, (void **)&T->d_wjobs, jobs.size() * sizeof(cm::WinoPackJob))) return 1;
    if (dev_alloc(m, (void **)&T->d_wblk2job, b2j.size() * sizeof(int))) return 1;
    CM_HIP(hipMemcpy(T->d_wjobs, jobs.data(), jobs.size() * sizeof(cm::WinoPackJob), hipMemcpyHostToDevice));
    CM_HIP(hipMemcpy(T->d_wblk2job, b2j.data(), b2j.size() * sizeof(int), hipMemcpyHostToDevice));
    T->wpack_blocks = (long long)b2j.size();
  }
  CM_HIP(cm::launch_wino_pack_jobs(T->opt.p, T->d_wjobs, T->d_wblk2job, T->wpack_blocks, st));
  // the split fragments of the inference forward follow the fp32 fragments just re-derived above
  for (Op &op : m->ops) {
    if (op.kind != OP_CONV) continue;
    if (op.d_wups_b6)
      CM_HIP(cm::launch_ups_b6_repack(op.ca.wfrag, op.ca.wpar_stride, op.d_wups_b6, op.wups_b6_stride, op.ca.Co, op.ca.C0, op.NB, st));
    if (op.d_wwino_b6) CM_HIP(cm::launch_wino_b6_repack(op.d_wwino, op.d_wwino_b6, op.wwino_floats, st));
    if (op.d_wqr_b6) CM_HIP(cm::launch_qr_b6_repack(op.d_wqr, op.d_wqr_b6, op.wqr_floats, op.ca.C0 + op.ca.C1, st));
    if (op.d_wfin) CM_HIP(cm::launch_fin_pack(T->opt.p + off_of(m, op.wname), op.d_wfin, op.ca.Co, 0, st));   // the last conv's column-packed fragments
  }
  for (auto &D : T->dg) {
    if (D.wwino_b6) CM_HIP(cm::launch_wino_b6_repack(D.wwino, D.wwino_b6, D.wwino_floats, st));
    if (D.qr) CM_HIP(cm::launch_qr_b6_repack(D.wqr, D.wqr_b6, D.wqr_floats, D.ca.C0, st));
  }
  return T->autocast ? repack_f16(m, st) : 0;
}

int train_setup(cm_model *m) {
  cm_train_state *T = m->train;
  const cm_unet_config &c = m->cfg;
  const size_t B = (size_t)c.max_batch;
  if (T->opt.init(m->params, {0}, false, [&](float **p, size_t n) { return dev_alloc(m, (void **)p, n * sizeof(float)); })) return 1;

  // ---- activation gradients, GroupNorm mean/rstd, maximal channel count ----
  int Cmax = 8;
  size_t Vfull = (size_t)m->L() * c.rows * c.cols;
  for (auto &a : m->acts) {
    if (dev_alloc(m, (void **)&a->g, B * a->V() * a->C * sizeof(float))) return 1;
    Cmax = std::max(Cmax, a->C);
  }
  for (Op &op : m->ops)
    if (op.kind == OP_GNFIN) {
      const int Ct = op.g0->C + (op.g1 ? op.g1->C : 0);
      Cmax = std::max(Cmax, Ct);
      if (dev_alloc(m, (void **)&op.gn_mr, B * 2 * Ct * sizeof(float))) return 1;
    }
  T->Cmax = Cmax;
  // scratch tensors: the largest (voxels x channels) product over the conv inputs / outputs
  size_t smax = Vfull * 8;
  for (Op &op : m->ops)
    if (op.kind == OP_CONV) {
      const size_t vin = (size_t)op.ca.Zs * op.ca.Ys * op.ca.Xs * (op.ca.par ? 8 : 1);
      smax = std::max(smax, vin * (size_t)(op.ca.C0 + op.ca.C1));
      smax = std::max(smax, (size_t)op.out_act->V() * (size_t)op.out_act->C);
    }
  for (float **b : {&T->scrA, &T->scrB, &T->scrC})
    if (dev_alloc(m, (void **)b, B * smax * sizeof(float))) return 1;
  if (dev_alloc(m, (void **)&T->tmp_bc, B * Cmax * sizeof(float))) return 1;
  {
    size_t need = 0;
    for (auto &op : m->ops)
      if (op.kind == OP_CONV) need += B * ((size_t)op.ca.Co + 2 * (size_t)(op.ca.C0 + op.ca.C1));
    T->bs_pool_floats = need;
    if (dev_alloc(m, (void **)&T->bs_pool, need * sizeof(float))) return 1;
  }
  if (dev_alloc(m, (void **)&T->vs_part, 16 * B * Cmax * sizeof(float))) return 1;
  if (dev_alloc(m, (void **)&T->dproj, B * m->nproj * sizeof(float))) return 1;
  if (dev_alloc(m, (void **)&T->train_temb, B * m->nproj * sizeof(float))) return 1;
  if (dev_alloc(m, (void **)&T->iota, B * sizeof(long long))) return 1;
  m->train_temb = T->train_temb; m->train_iota = T->iota;
  {
    std::vector<long long> io(B);
    for (size_t i = 0; i < B; ++i) io[i] = (long long)i;
    CM_HIP(hipMemcpy(T->iota, io.data(), B * sizeof(long long), hipMemcpyHostToDevice));
  }
  if (dev_alloc(m, (void **)&T->gnb_part, B * MAX_SLICES * Cmax * 2 * sizeof(float))) return 1;
  if (dev_alloc(m, (void **)&T->gnb_coef, B * 3 * Cmax * sizeof(float))) return 1;
  if (dev_alloc(m, (void **)&T->gnb_dgb, B * 2 * Cmax * sizeof(float))) return 1;
  const int te = c.base_channels, tx = c.base_channels * c.time_multiple;
  if (dev_alloc(m, (void **)&T->time_ws, B * (te + 6 * (size_t)tx) * sizeof(float))) return 1;
  if (dev_alloc(m, (void **)&T->dWd_all, (size_t)m->nproj * tx * sizeof(float))) return 1;
  if (dev_alloc(m, (void **)&T->dbd_all, (size_t)m->nproj * sizeof(float))) return 1;
  const size_t per = (size_t)m->per_sample();
  if (dev_alloc(m, (void **)&T->xt, B * per * sizeof(float))) return 1;
  if (dev_alloc(m, (void **)&T->pred, B * per * sizeof(float))) return 1;
  if (dev_alloc(m, (void **)&T->eps_dev, B * per * sizeof(float))) return 1;
  T->wpart_floats = (size_t)64 << 20;  // 256 MiB of partial weight gradients
  if (dev_alloc(m, (void **)&T->wpart, T->wpart_floats * sizeof(float))) return 1;

  // ---- index maps of every derived forward tensor + the data-gradient launches ----
  T->dg.resize(m->ops.size());
  for (size_t oi = 0; oi < m->ops.size(); ++oi) {
    Op &op = m->ops[oi];
    if (op.kind == OP_GNFIN) {
      if (add_derived(m, const_cast<float *>(op.gamma), flat_index(m, op.gname), 1)) return 1;
      if (add_derived(m, const_cast<float *>(op.beta), flat_index(m, op.bename), 1)) return 1;
      continue;
    }
    if (op.kind == OP_ATTNBLK) {
      // reference-layout weight copies of the fused attention block follow the master weights too
      if (add_derived(m, op.d_win, flat_index(m, op.win_name), 1) || add_derived(m, op.d_wout, flat_index(m, op.wout_name), 1)) return 1;
      continue;
    }
    if (op.kind != OP_CONV) continue;
    const Param &w = P(m, op.wname);
    const int Co = (int)w.shape[0], Ci = (int)w.shape[1], nt = op.ref_taps;
    const int Ci_pad = op.ca.C0 + op.ca.C1;
    const std::vector<int> ii = ref_index_internal(m, op.wname, Co, Ci, nt);
    // forward packed weights
    if (op.ca.par) {
      long long stride = 0;
      const std::vector<Src8> all = pack_parity_classes(parity_sources(ii, Co, Ci), &stride, [&](const Src8 *s8) {
        return pack_conv(s8, Co, Ci, 8, Ci_pad, op.ca.CK, op.NB, kNoSrc8);
      });
      if (add_derived(m, const_cast<float *>(op.ca.wfrag), all)) return 1;
    } else {
      if (add_derived(m, const_cast<float *>(op.ca.wfrag), pack_conv(ii.data(), Co, Ci, nt, Ci_pad, op.ca.CK, op.NB, -1), 1)) return 1;
    }
    if (op.d_s2w) {
      // inference-only fused skip conv: keep its packed weights / summed bias in step with the master copy
      const Param &w2 = P(m, op.skip_w);
      const int Ci2 = (int)w2.shape[1];
      const std::vector<int> i2 = ref_index_internal(m, op.skip_w, Co, Ci2, 1);
      if (add_derived(m, op.d_s2w, pack_conv(i2.data(), Co, Ci2, 1, Ci2, 32, op.NB, -1), 1)) return 1;
      const int TNf = 32 * op.NB, cpf = (op.ca.Co + TNf - 1) / TNf * TNf;
      std::vector<int> ibf((size_t)cpf * 2, -1);
      for (int i = 0; i < Co; ++i) { ibf[2 * i] = (int)(off_of(m, op.bname) + i); ibf[2 * i + 1] = (int)(off_of(m, op.skip_b) + i); }
      if (add_derived(m, op.d_bias_fused, ibf, 2)) return 1;
    }
    if (op.wino) {
      if (add_derived_wino(m, op.d_wwino, ii, Co, Ci, Ci_pad)) return 1;
    }
    if (op.qr) {
      // whole-sample quarter-resolution kernel of the inference plan
      if (add_derived(m, op.d_wqr, pack_qr(ii, Co, Ci), 1)) return 1;
      if (op.d_wqr_skip) {
        const int Ci2 = (int)P(m, op.skip_w).shape[1];
        if (add_derived(m, op.d_wqr_skip, pack_qr_skip(ref_index_internal(m, op.skip_w, Co, Ci2, 1).data(), Co, Ci2), 1)) return 1;
      }
    }
    if (op.first_k && add_derived(m, op.d_wfirst, pack_first(ii.data(), Co, Ci, op.first_cin, -1), 1)) return 1;
    if (op.small_n && add_derived(m, op.d_wsmall, pack_small(ii.data(), Co, Ci, Ci_pad, op.ca.CK, op.small_nco, -1), 1)) return 1;
    {
      const int TN = 32 * op.NB, co_pad = (op.ca.Co + TN - 1) / TN * TN;
      std::vector<int> ib((size_t)co_pad, -1);
      for (int i = 0; i < Co; ++i) ib[i] = (int)(off_of(m, op.bname) + i);
      if (add_derived(m, const_cast<float *>(op.ca.bias), ib, 1)) return 1;
    }
    // ---- data gradient: dA[.., Ctot_in] = conv(dY, W'),  W'[ci][co][t'] = W[co][ci][flip t'] ----
    cm_train_state::Dgrad &D = T->dg[oi];
    const bool first = (op.in0 == m->x8_act);
    const int Cy = op.out_act->C;  // channel stride of dY (>= Co)
    if (!first) {
      D.have = true;
      std::vector<int> src((size_t)Ci * Co * nt);
      for (int ci = 0; ci < Ci; ++ci)
        for (int co = 0; co < Co; ++co)
          for (int t = 0; t < nt; ++t) src[((size_t)ci * Co + co) * nt + t] = ii[((size_t)co * Ci + ci) * nt + (nt - 1 - t)];
      cm::ConvArgs &a = D.ca;
      a = cm::ConvArgs{};
      a.C0 = Cy; a.C1 = 0; a.Co = Ci;
      a.ntaps = nt; a.td = nt == 27 ? 3 : 1; a.stride = 1; a.ups = 0; a.par = 0; a.ks = 1;
      // spatial dims: the data gradient lives on the conv's INPUT grid (stride-2: zero-stuffed dY;
      // upsample: the upsampled grid, pooled afterwards)
      const int up = op.ca.par ? 2 : 1;
      a.Zs = a.Zo = op.ca.Zs * up; a.Ys = a.Yo = op.ca.Ys * up; a.Xs = a.Xo = op.ca.Xs * up;
      a.out_cs = Ci_pad; a.CK = pick_ck(Cy, 0);
      a.nch0 = Cy / a.CK; a.nch1 = 0;
      D.NB = Ci > 32 ? 2 : 1;
      const std::vector<int> pidx = pack_conv(src.data(), Ci, Co, nt, Cy, a.CK, D.NB, -1);
      if (dev_alloc(m, (void **)&D.wfrag, pidx.size() * sizeof(float))) return 1;
      if (add_derived(m, D.wfrag, pidx, 1, true)) return 1;
      const int TN = 32 * D.NB, cop = (Ci + TN - 1) / TN * TN;
      std::vector<float> zb((size_t)cop, 0.f);
      if (upload(m, zb, &D.zero_bias)) return 1;
      a.wfrag = D.wfrag; a.bias = D.zero_bias;
      int wz = 0, wy = 0, wx = 0;
      if (nt == 27 && Cy % 16 == 0 && Ci % 32 == 0 && Ci == Ci_pad && (long)a.Zo * a.Yo * a.Xo > 64 &&
          cm::conv_wino_pick(a.Zo, a.Yo, a.Xo, &wz, &wy, &wx) && !cm::diag_env("CM_NO_WINO")) {
        // the data gradient of a 3x3x3 conv is a stride-1 3x3x3 conv of dY with the flipped / transposed weights:
        // same Winograd kernel, its transformed weights re-derived from the master copy after every update
        D.wino = true;
        const size_t nel = (size_t)((Ci + 31) / 32) * (Cy / 16) * 4 * 24 * 64 * 4;
        if (dev_alloc(m, (void **)&D.wwino, nel * sizeof(float))) return 1;
        if (add_derived_wino(m, D.wwino, src, Ci, Co, Cy)) return 1;
        D.wwino_floats = (long long)nel;
        // fp32 plan: the data gradient takes the six-term bf16 form wherever the forward's tile does (exact three-way
        // splits, fp32 accumulate: fp32-level products at 2.7x the matrix rate)
        if (m->precision != CM_PRECISION_F16 && !cm::diag_env("CM_NO_WINO_B6") && !cm::diag_env("CM_NO_TRAIN_B6") &&
            cm::conv_wino_b6_ok(wz, wy, wx, Ci, a.Zo) && dev_alloc(m, (void **)&D.wwino_b6, nel * 3 / 2 * sizeof(float)))
          return 1;
        a.bs = 1; a.bz = wz; a.by = wy; a.bx = wx;
        a.ntz = a.Zo / wz; a.nty = (a.Yo + wy - 1) / wy; a.ntx = (a.Xo + wx - 1) / wx;
        if (!cm::conv_wino_ok(a)) return fail("Winograd data-gradient tile does not fit %s", op.label.c_str());
      } else if (tune_launch(m, a, D.MB, D.NB, D.d_hv, D.d_mt, false)) return 1;
      // quarter resolution (two planes): forward and data gradient of the training step on conv_qr2's six-term form
      if (op.qr && op.d_wqr_b6 && nt == 27 && Cy == Co && Co % 64 == 0 && Ci % 32 == 0 && Ci == Ci_pad && a.Zo == 2 &&
          a.Yo * a.Xo <= 64 && 8 * (a.Yo + 2) * (a.Xo + 2) <= 64 * 9 && m->precision != CM_PRECISION_F16 && !cm::diag_env("CM_NO_TRAIN_QR")) {
        op.train_qr = true;
        const int ntn = Ci / 32, cw = Co / 8, nsw = (cw + 15) >> 4;
        const std::vector<int> wq = pack_qr(src, Ci, Co);                 // dgrad output channels Ci, input channels Co (= Cy)
        D.wqr_floats = (long long)wq.size();
        if (dev_alloc(m, (void **)&D.wqr, wq.size() * sizeof(float))) return 1;
        if (add_derived(m, D.wqr, wq, 1, true)) return 1;
        const size_t n6 = (size_t)ntn * 8 * nsw * 9 * 3 * 3 * 64 * 4;      // pack_qr_b6 order, padded steps stay zero
        if (dev_alloc(m, (void **)&D.wqr_b6, n6 * sizeof(float))) return 1;
        CM_HIP(hipMemset(D.wqr_b6, 0, n6 * sizeof(float)));
        D.qr = true;
      }
    }
    // weight-gradient geometry (one sample per tile; the parity-mode upsample conv is taken in
    // its plain 27-tap form over the materialised upsampled input)
    if (op.wino && Ci % 32 == 0 && Co % 32 == 0 && !cm::diag_env("CM_NO_WINO_WGRAD")) {
      D.wwg = true;
      D.wwa = op.ca;
      cm::ConvArgs &w2 = D.wwa;
      w2.bs = 1; w2.ks = 1;
      if (!cm::conv_wino_pick(w2.Zo, w2.Yo, w2.Xo, &w2.bz, &w2.by, &w2.bx)) return fail("no Winograd tile for the weight gradient of %s", op.label.c_str());
      w2.ntz = w2.Zo / w2.bz; w2.nty = (w2.Yo + w2.by - 1) / w2.by; w2.ntx = (w2.Xo + w2.bx - 1) / w2.bx;
    }
    {
      D.own_wgeom = true;
      cm::ConvArgs &wa = D.wa;
      wa = op.ca;
      wa.ks = 1;   // (parity-mode upsample convs keep their 2x2x2 parity form: 8 taps on the low-resolution input)
      if (tune_launch(m, wa, D.wMB, 1, D.w_hv, D.w_mt, true)) return 1;
      // two-plane grids (quarter resolution): z-split row order -- plane z in row block z -- so that the kernel can
      // skip the z tap on the padding plane, as the forward's z-split form does (cm_conv.hip)
      if (wa.ntaps == 27 && wa.stride == 1 && !wa.par && !wa.ups && wa.Zo == 2 && wa.Zs == 2 && wa.bz == 2 && wa.by * wa.bx <= 32 &&
          !cm::diag_env("CM_NO_WGRAD_ZSPLIT")) {
        std::vector<int> mt(64, -1);
        for (int z = 0; z < 2; ++z)
          for (int y = 0; y < wa.by; ++y)
            for (int x = 0; x < wa.bx; ++x) mt[(size_t)z * 32 + y * wa.bx + x] = (z << 18) | (y << 9) | x;
        if (dev_alloc(m, (void **)&D.w_mt, mt.size() * sizeof(int))) return 1;
        CM_HIP(hipMemcpy(D.w_mt, mt.data(), mt.size() * sizeof(int), hipMemcpyHostToDevice));
        wa.mtab = D.w_mt;
        wa.zsplit = 1;
        D.wMB = 2;
      }
    }
  }
  // time-embedding MLP copies
  {
    if (add_derived(m, m->d_time[1], flat_index(m, "time_embeddings.time_blocks.1.weight"), 1)) return 1;
    if (add_derived(m, m->d_time[2], flat_index(m, "time_embeddings.time_blocks.1.bias"), 1)) return 1;
    if (add_derived(m, m->d_time[3], flat_index(m, "time_embeddings.time_blocks.3.weight"), 1)) return 1;
    if (add_derived(m, m->d_time[4], flat_index(m, "time_embeddings.time_blocks.3.bias"), 1)) return 1;
    std::vector<int> wd, bd;
    auto visit = [&](const BlockDesc &b) {
      if (b.kind != 0) return;
      for (int v : flat_index(m, b.prefix + ".dense_1.weight")) wd.push_back(v);
      for (int v : flat_index(m, b.prefix + ".dense_1.bias")) bd.push_back(v);
    };
    for (auto &b : m->enc) visit(b);
    for (auto &b : m->bott) visit(b);
    for (auto &b : m->dec) visit(b);
    if (add_derived(m, m->d_time[5], wd, 1)) return 1;
    if (add_derived(m, m->d_time[6], bd, 1)) return 1;
  }
  // every derived tensor (forward fragments included) is rebuilt from the master copy by the same
  // kernel that re-packs after an optimizer step, so a handle resumed from a checkpoint continues
  // bit-identically to the handle that wrote it
  if (repack_all(m, m->stream)) return 1;
  CM_HIP(hipDeviceSynchronize());
  return 0;
}

// accumulate a channels-last gradient slice into an activation's gradient buffer
int accum_act(cm_model *m, const Act *a, const float *src, int src_cs, int B, hipStream_t st) {
  CM_HIP(cm::launch_add_into(a->g, a->C, src, src_cs, a->C, (long long)B * a->V(), m->train->gset.insert(a).second ? 0 : 1, st));
  return 0;
}

int backward_ops_impl(cm_model *m, int B, hipStream_t st);
// Weight-gradient launches run on a second stream (backward_ops_impl): an early error return must not leave them queued or
// running behind the caller's back -- a caller that retries, reads gradients or destroys the handle would race with kernels
// that still read activations and write the gradient / partial buffers.  Join that stream before reporting the failure.
int backward_ops(cm_model *m, int B, hipStream_t st) {
  const int rc = backward_ops_impl(m, B, st);
  if (rc && m->lane_stream[1] && m->lane_stream[1] != st) (void)hipStreamSynchronize(m->lane_stream[1]);
  return rc;
}

int backward_ops_impl(cm_model *m, int B, hipStream_t st) {
  cm_train_state *T = m->train;
  std::set<const Act *> &gset = T->gset;
  gset = {m->act_by_name.at("final")};      // written by mse_grad
  T->bs_cursor = 0;
  if (!T->bs_ready) {
    // the deferred job tables are appended during the first COMPLETE pass: a first pass that returned early (an
    // allocation failure, a partial buffer too small) must not leave half a table behind for the next call to extend
    T->bs_jobs.clear();
    T->vs_jobs.clear();
    T->bs_maxC = T->vs_maxC = 0;
  }
  CM_HIP(hipMemsetAsync(T->dproj, 0, (size_t)B * m->nproj * sizeof(float), st));
  static const bool one_stream = cm::diag_env("CM_WGRAD_ONE_STREAM") != nullptr;
  hipStream_t wst = (one_stream || !m->lane_stream[1]) ? st : m->lane_stream[1];
  if (wst != st && !T->ev_dy) {
    CM_HIP(hipEventCreateWithFlags(&T->ev_dy, hipEventDisableTiming));
    CM_HIP(hipEventCreateWithFlags(&T->ev_wdone, hipEventDisableTiming));
  }
  static const bool sync_ops = cm::diag_env("CM_SYNC_OPS") != nullptr;   // debugging: name every op and drain the device after it
  for (int oi = (int)m->ops.size() - 1; oi >= 0; --oi) {
    Op &op = m->ops[oi];
    if (sync_ops) {
      const hipError_t e = hipDeviceSynchronize();
      fprintf(stderr, "[cm] backward reaches op %d %s (%s)\n", oi, op.label.c_str(), hipGetErrorString(e));
      fflush(stderr);
    }
    if (op.kind == OP_ATTN) {
      // qkv is the op's input tensor, aout its output: locate their activations by pointer
      Act *qa = nullptr, *oa = nullptr;
      for (auto &a : m->acts) { if (a->d == op.qkv) qa = a.get(); if (a->d == op.aout) oa = a.get(); }
      if (!qa || !oa || !gset.count(oa)) return fail("attention backward: missing gradient");
      const size_t need = cm::attn_bwd_scratch_floats(m->cfg.max_batch, op.S, op.E, ATTN_HEADS);
      if (need > T->attn_big_floats) {              // (large token counts only: the S x S matrices go to a global slab)
        if (dev_alloc(m, (void **)&T->attn_big, need * sizeof(float))) return 1;
        T->attn_big_floats = need;
      }
      CM_HIP(cm::launch_attn_bwd(op.qkv, oa->g, qa->g, B, op.S, op.E, ATTN_HEADS, need ? T->attn_big : nullptr, st));
      gset.insert(qa);
      continue;
    }
    if (op.kind != OP_CONV) continue;
    const Act *out = op.out_act;
    if (!gset.count(out)) return fail("backward: no gradient reached %s", op.label.c_str());
    const float *dY = out->g;
    const int Cy = out->C, Co = op.ca.Co;
    const int Vo = out->V();
    cm_train_state::Dgrad &D = T->dg[oi];
    // residual branch
    if (op.resid_act && accum_act(m, op.resid_act, dY, Cy, B, st)) return 1;
    // bias gradient and the broadcast time-embedding term
    float *bc = T->bs_pool + T->bs_cursor;
    T->bs_cursor += (size_t)m->cfg.max_batch * Co;
    if (T->bs_cursor > T->bs_pool_floats) return fail("batch-sum pool overflow");
    // (dY = the output activation's gradient buffer stays intact until the end of the pass: every act owns its buffer
    // and all of its consumers have already contributed -- so its voxel sum can wait for the one job-table launch)
    if (!T->bs_ready) {
      T->vs_jobs.push_back({dY, Vo, Co, Cy, bc, Co, op.temb_off >= 0 ? T->dproj + op.temb_off : nullptr, m->nproj});
      T->vs_maxC = std::max(T->vs_maxC, Co);
      T->bs_jobs.push_back({bc, grad_of(m, op.bname), Co, Co});
      T->bs_maxC = std::max(T->bs_maxC, Co);
    }
    // weight gradient: off the critical path (only the optimizer reads it), so its launches go to a second stream and fill
    // the tails / launch gaps of the data-gradient chain.  Inputs: dY (final: every consumer of this op's output has already
    // contributed, and nothing writes it again in this pass) and forward activations; outputs: the parameter's gradient and
    // the partial buffer, which only this stream touches.
    if (wst != st) {
      CM_HIP(hipEventRecord(T->ev_dy, st));
      CM_HIP(hipStreamWaitEvent(wst, T->ev_dy, 0));
    }
    if (D.wwg) {
      cm::ConvArgs wa = D.wwa;
      wa.B = B;
      if (op.pm_off >= 0) { wa.pm = m->dropmask + op.pm_off; wa.pm_stride = m->nproj; }
      const int ncb = (Co + 31) / 32, nkb = (wa.C0 + wa.C1 + 31) / 32;
      const long ntile = (long)wa.ntz * wa.nty * wa.ntx * B;
      const size_t per_g = (size_t)ncb * nkb * 48 * 1024;
      static const int wino_wgs = cm::diag_env("CM_WGRAD_WINO_WGS") ? atoi(cm::diag_env("CM_WGRAD_WINO_WGS")) : 192;   // (with the weight gradients on their own stream: 128 / 192 / 256 / 512 -> 14.63 / 13.59 / 13.69 / 13.88 ms per step)
      int G = (int)std::min<long>(ntile, std::max(1, wino_wgs / (ncb * nkb)));      // one workgroup per CU (80 KB image, 192 accumulators)
      G = (int)std::min<size_t>((size_t)G, T->wpart_floats / per_g);
      if (G < 1) return fail("wgrad partial buffer too small");
      const Param &w = P(m, op.wname);
      if (T->autocast) CM_HIP(cm::launch_wgrad_wino_f16(wa, dY, Cy, T->wpart, G, ncb, nkb, wst));
      else CM_HIP(cm::launch_wgrad_wino(wa, dY, Cy, T->wpart, G, ncb, nkb, wst));
      CM_HIP(cm::launch_wgrad_wino_reduce(T->wpart, G, ncb, nkb, (int)w.shape[0], (int)w.shape[1], grad_of(m, op.wname), wst));
    } else if (op.ref_taps == 27 && op.ca.stride == 1 && !op.ca.par && !op.ca.ups && op.pm_off < 0 && !cm::diag_env("CM_NO_WGRAD_PACK") &&
               ((Co == 32 && !op.in1 && op.in0->C == 8 && !op.ca.gn) || (Co <= 4 && op.ca.C0 + op.ca.C1 == 32 && !op.in1))) {
      // few channels on one side (first / last conv of the UNet): taps packed with the narrow side into the MFMA columns
      const Param &w = P(m, op.wname);
      const bool last = Co <= 4;
      cm::WgradPackArgs pa{};
      if (last) {
        pa.wide = op.in0->d; pa.wide_cs = op.in0->C; pa.gn = op.ca.gn; pa.silu = op.ca.silu;
        pa.narrow = dY; pa.narrow_cs = Cy; pa.cn_valid = Co; pa.mirror = 1;
      } else {
        pa.wide = dY; pa.wide_cs = Cy; pa.gn = nullptr; pa.silu = 0;
        pa.narrow = op.in0->d; pa.narrow_cs = op.in0->C; pa.cn_valid = (int)w.shape[1]; pa.mirror = 0;
      }
      const int CN = last ? 4 : 8;
      pa.B = B; pa.Z = op.ca.Zo; pa.Y = op.ca.Yo; pa.X = op.ca.Xo;
      pa.bz = std::min(pa.Z, 8); pa.by = std::min(pa.Y, 4); pa.bx = std::min(pa.X, 6);
      if ((pa.bz * pa.by * pa.bx) & 1) pa.bx += 1;   // (an even number of rows: voxel pairs; rows outside the grid are zero)
      pa.ntz = (pa.Z + pa.bz - 1) / pa.bz; pa.nty = (pa.Y + pa.by - 1) / pa.by; pa.ntx = (pa.X + pa.bx - 1) / pa.bx;
      const long ntile = (long)B * pa.ntz * pa.nty * pa.ntx;
      const size_t per_g = (size_t)((27 * CN + 31) / 32) * 1024;
      int G = (int)std::min<long>(ntile, 256);
      G = (int)std::min<size_t>((size_t)G, T->wpart_floats / per_g);
      if (G < 1) return fail("wgrad partial buffer too small");
      pa.part = T->wpart;
      CM_HIP(cm::launch_wgrad_pack(pa, CN, G, wst));
      CM_HIP(cm::launch_wgrad_pack_reduce(T->wpart, G, CN, pa.cn_valid, pa.mirror, (int)w.shape[0], (int)w.shape[1], grad_of(m, op.wname), wst));
    } else if (D.wa.par && !D.wa.gn && op.pm_off < 0 && !cm::diag_env("CM_NO_WGRAD_PAR")) {
      // upsample convs: parity-form kernel with all 8 tap blocks per wave
      cm::ConvArgs wa = D.wa;
      wa.B = B;
      wa.bz = std::min(wa.Zs, 4); wa.by = std::min(wa.Ys, 6); wa.bx = std::min(wa.Xs, wa.Zs <= 2 ? 9 : 6);
      wa.ntz = (wa.Zs + wa.bz - 1) / wa.bz; wa.nty = (wa.Ys + wa.by - 1) / wa.by; wa.ntx = (wa.Xs + wa.bx - 1) / wa.bx;
      const int Ctot = wa.C0 + wa.C1;
      const int ncb = (Co + 31) / 32, nkb = (Ctot + 31) / 32;
      const long ntile = (long)wa.ntz * wa.nty * wa.ntx * B;
      const size_t per_g = (size_t)ncb * nkb * 64 * 1024;
      static const int wgs_par = cm::diag_env("CM_WGRAD_PAR_WGS") ? atoi(cm::diag_env("CM_WGRAD_PAR_WGS")) : 1024;
      int G = (int)std::min<long>(ntile, std::max(2, wgs_par / (8 * ncb * nkb)));
      G = (int)std::min<size_t>((size_t)G, T->wpart_floats / per_g);
      if (G < 1) return fail("wgrad partial buffer too small");
      const Param &w = P(m, op.wname);
      CM_HIP(cm::launch_wgrad_par(wa, dY, Cy, T->wpart, G, ncb, nkb, wst));
      CM_HIP(cm::launch_wgrad_reduce_par(T->wpart, G, ncb, nkb, (int)w.shape[0], (int)w.shape[1], grad_of(m, op.wname), wst));
    } else if (op.ref_taps == 1 && op.ca.stride == 1 && !op.ca.par && !op.ca.ups && !cm::diag_env("CM_NO_WGRAD_1X1")) {
      // 1x1x1 convs (skip convs, attention projections): flat-row kernel, NKB input blocks per workgroup
      cm::ConvArgs wa = D.wa;
      wa.B = B;
      if (op.pm_off >= 0) { wa.pm = m->dropmask + op.pm_off; wa.pm_stride = m->nproj; }
      const int Ctot = wa.C0 + wa.C1;
      const int ncb = (Co + 31) / 32, nkb = (Ctot + 31) / 32;
      const int NKB = nkb % 4 == 0 ? 4 : (nkb % 3 == 0 ? 3 : (nkb % 2 == 0 ? 2 : 1));
      const long long N = (long long)B * Vo;
      const size_t per_g = (size_t)ncb * nkb * 1024;
      static const int wgs_1x1 = cm::diag_env("CM_WGRAD_1X1_WGS") ? atoi(cm::diag_env("CM_WGRAD_1X1_WGS")) : 768;
      int G = (int)std::min<long long>((N + 127) / 128, std::max(4, wgs_1x1 / (ncb * (nkb / NKB))));
      G = (int)std::min<size_t>((size_t)G, T->wpart_floats / per_g);
      if (G < 1) return fail("wgrad partial buffer too small");
      const Param &w = P(m, op.wname);
      CM_HIP(cm::launch_wgrad_1x1(wa, dY, Cy, Vo, T->wpart, G, ncb, nkb, NKB, wst));
      CM_HIP(cm::launch_wgrad_reduce(T->wpart, G, ncb, nkb, 1, (int)w.shape[0], (int)w.shape[1], grad_of(m, op.wname), wst, 1));
    } else {
      cm::ConvArgs wa = D.wa;
      const int wMB = D.wMB;
      wa.B = B; wa.nts = B; wa.ks = 1;
      if (op.pm_off >= 0) { wa.pm = m->dropmask + op.pm_off; wa.pm_stride = m->nproj; }
      const int Ctot = wa.C0 + wa.C1;
      const int ncb = (Co + 31) / 32, nkb = (Ctot + 31) / 32;
      const long ntile = (long)wa.ntz * wa.nty * wa.ntx * B;
      const size_t per_g = (size_t)ncb * nkb * (wa.par ? 64 : (op.ref_taps == 1 ? 4 : op.ref_taps)) * 1024;   // parity form: 8 classes x 8 taps per group; 1x1x1: 4 per-wave partials
      // one full round of resident workgroups, as few partial copies as that allows
      static const int wg_target = cm::diag_env("CM_WGRAD_WGS") ? atoi(cm::diag_env("CM_WGRAD_WGS")) : 256;   // two workgroups per CU fit (62 KB LDS each): 512 = one even round (768: 26.0 ms, 512: 23.2 ms per step)
      int G = (int)std::min<long>(ntile, std::max(4, wg_target / (ncb * nkb)));
      G = (int)std::min<size_t>((size_t)G, T->wpart_floats / per_g);
      if (G < 1) return fail("wgrad partial buffer too small");
      const Param &w = P(m, op.wname);
      static const bool no_zs_kernel = cm::diag_env("CM_NO_WGRAD_ZS_KERNEL") != nullptr;
      if (wa.zsplit && !no_zs_kernel && cm::wgrad_zs_ok(wa)) {
        // two-plane grids: the dedicated kernel (two input blocks per workgroup, arithmetic coordinates, one load batch per tile)
        const int nkg = (nkb + 1) / 2;
        static const int zs_wgs = cm::diag_env("CM_WGRAD_ZS_WGS") ? atoi(cm::diag_env("CM_WGRAD_ZS_WGS")) : 128;   // one workgroup per CU, fewest partial copies (128 / 256 / 512 / 1024: 16.84 / 16.30 / 16.46 / 16.75 ms per step)
        int Gz = (int)std::min<long>(ntile, std::max(4, zs_wgs / (ncb * nkg)));
        Gz = (int)std::min<size_t>((size_t)Gz, T->wpart_floats / per_g);
        CM_HIP(cm::launch_wgrad_zs(wa, dY, Cy, T->wpart, Gz, ncb, nkb, wst));
        CM_HIP(cm::launch_wgrad_reduce(T->wpart, Gz, ncb, nkb, op.ref_taps, (int)w.shape[0], (int)w.shape[1], grad_of(m, op.wname), wst));
      } else {
        CM_HIP(cm::launch_wgrad(wa, wMB, dY, Cy, T->wpart, G, ncb, nkb, wst));
        if (wa.par)
          CM_HIP(cm::launch_wgrad_reduce_par(T->wpart, G, ncb, nkb, (int)w.shape[0], (int)w.shape[1], grad_of(m, op.wname), wst));
        else
          CM_HIP(cm::launch_wgrad_reduce(T->wpart, G, ncb, nkb, op.ref_taps, (int)w.shape[0], (int)w.shape[1],
                                         grad_of(m, op.wname), wst));
      }
    }
    if (!D.have) continue;  // first conv: its input is data
    // data gradient into scrA [B][Vin][Ctot]
    cm::ConvArgs da = D.ca;
    da.B = B; da.nts = (B + da.bs - 1) / da.bs;
    const float *dysrc = dY;
    if (op.ca.stride == 2) {
      CM_HIP(cm::launch_zero_stuff2(dY, T->scrB, B, op.ca.Zo, op.ca.Yo, op.ca.Xo, Cy, st));
      dysrc = T->scrB;
    }
    da.src0 = dysrc; da.out = T->scrA; da.tidx = m->tbuf;
    if (D.qr) {
      cm::QrArgs q{};
      q.src0 = dysrc; q.C0 = da.C0; q.raw = 1; q.groups = 8;
      q.wq = D.wqr; q.wq6 = D.wqr_b6; q.bias = D.zero_bias; q.tidx = m->tbuf;
      q.out = T->scrA; q.out_cs = da.out_cs; q.Co = da.Co; q.B = B; q.Y = da.Yo; q.X = da.Xo;
      if (!cm::conv_qr2_b6_ok(q)) return fail("quarter-resolution data gradient of %s: no six-term form", op.label.c_str());
      CM_HIP(cm::launch_conv_qr(q, st));
    } else if (D.wino) {
      da.wfrag = D.wwino;
      const bool f16 = T->autocast && D.wwino16;
      if (f16) da.wfrag = D.wwino16;
      else if (D.wwino_b6) { da.wfrag = D.wwino_b6; da.f16 = 2; }
      CM_HIP(cm::launch_conv_wino(da, f16, st));
    } else {
      CM_HIP(cm::launch_conv(da, D.MB, D.NB, st));
    }
    const int Ctot = op.ca.C0 + op.ca.C1;
    if (op.ca.par) {
      const Act *in = op.in0;
      CM_HIP(cm::launch_sumpool2(T->scrA, in->g, B, op.ca.Zs, op.ca.Ys, op.ca.Xs, in->C, gset.insert(in).second ? 0 : 1, st));
    } else if (op.gn_op >= 0) {
      Op &gop = m->ops[op.gn_op];
      cm::GnbArgs ga{};
      ga.x0 = op.in0->d; ga.x1 = op.in1 ? op.in1->d : nullptr; ga.C0 = op.ca.C0; ga.C1 = op.ca.C1;
      ga.dA = T->scrA; ga.dA_cs = Ctot;
      ga.gn = gop.gn_out; ga.mr = gop.gn_mr; ga.gamma = gop.gamma;
      ga.pm = op.pm_off >= 0 ? m->dropmask + op.pm_off : nullptr; ga.pm_stride = m->nproj;
      ga.silu = op.ca.silu;
      ga.V = op.in0->V(); ga.B = B; ga.groups = GN_GROUPS;
      ga.nsl = std::max(1, std::min(MAX_SLICES, ga.V / 128));
      float *dgb = T->bs_pool + T->bs_cursor;
      T->bs_cursor += (size_t)m->cfg.max_batch * 2 * Ctot;
      if (T->bs_cursor > T->bs_pool_floats) return fail("batch-sum pool overflow");
      ga.part = T->gnb_part; ga.coef = T->gnb_coef; ga.dgb = dgb;
      ga.g1 = op.in1 ? op.in1->g : nullptr; ga.acc1 = (op.in1 && gset.count(op.in1)) ? 1 : 0;
      ga.g0 = op.in0->g; ga.acc0 = gset.insert(op.in0).second ? 0 : 1;
      if (op.in1) gset.insert(op.in1);
      CM_HIP(cm::launch_gn_backward(ga, st));
      if (!T->bs_ready) {
        T->bs_jobs.push_back({dgb, grad_of(m, gop.gname), Ctot, 2 * Ctot});
        T->bs_jobs.push_back({dgb + Ctot, grad_of(m, gop.bename), Ctot, 2 * Ctot});
        T->bs_maxC = std::max(T->bs_maxC, Ctot);
      }
    } else {
      if (accum_act(m, op.in0, T->scrA, Ctot, B, st)) return 1;
      if (op.in1 && accum_act(m, op.in1, T->scrA + op.ca.C0, Ctot, B, st)) return 1;
    }
  }
  if (wst != st) {                                 // every weight gradient is complete before the optimizer reads it
    CM_HIP(hipEventRecord(T->ev_wdone, wst));
    CM_HIP(hipStreamWaitEvent(st, T->ev_wdone, 0));
  }
  // the deferred batch reductions (bias, gamma, beta gradients) in one launch
  if (!T->bs_ready) {
    if (dev_alloc(m, (void **)&T->d_bs_jobs, T->bs_jobs.size() * sizeof(cm::BsumJob))) return 1;
    if (dev_alloc(m, (void **)&T->d_vs_jobs, T->vs_jobs.size() * sizeof(cm::VsumJob))) return 1;
    CM_HIP(hipMemcpyAsync(T->d_bs_jobs, T->bs_jobs.data(), T->bs_jobs.size() * sizeof(cm::BsumJob), hipMemcpyHostToDevice, st));
    CM_HIP(hipMemcpyAsync(T->d_vs_jobs, T->vs_jobs.data(), T->vs_jobs.size() * sizeof(cm::VsumJob), hipMemcpyHostToDevice, st));
    CM_HIP(hipStreamSynchronize(st));
    T->bs_ready = true;
  }
  CM_HIP(cm::launch_voxel_sum_jobs(T->d_vs_jobs, (int)T->vs_jobs.size(), B, T->vs_maxC, st));
  CM_HIP(cm::launch_batch_sum_jobs(T->d_bs_jobs, (int)T->bs_jobs.size(), B, T->bs_maxC, st));
  // time-embedding path
  const cm_unet_config &c = m->cfg;
  cm::TimeBwdArgs ta{};
  ta.table = m->d_time[0]; ta.t = m->tbuf;
  ta.W1 = m->d_time[1]; ta.b1 = m->d_time[2]; ta.W2 = m->d_time[3]; ta.b2 = m->d_time[4]; ta.Wd = m->d_time[5]; ta.bd = m->d_time[6];
  ta.te = c.base_channels; ta.tx = c.base_channels * c.time_multiple; ta.nproj = m->nproj; ta.B = B;
  ta.dproj = T->dproj; ta.ws = T->time_ws;
  ta.dW1 = grad_of(m, "time_embeddings.time_blocks.1.weight"); ta.db1 = grad_of(m, "time_embeddings.time_blocks.1.bias");
  ta.dW2 = grad_of(m, "time_embeddings.time_blocks.3.weight"); ta.db2 = grad_of(m, "time_embeddings.time_blocks.3.bias");
  ta.dWd = T->dWd_all; ta.dbd = T->dbd_all;
  CM_HIP(cm::launch_time_bwd(ta, st));
  if (!T->d_cp_jobs) {            // the per-block slices -> their parameters' gradient slots: one job-table launch
    std::vector<cm::CopyJob> jobs;
    int off = 0;
    auto visit = [&](const BlockDesc &b) {
      if (b.kind != 0) return;
      jobs.push_back({grad_of(m, b.prefix + ".dense_1.weight"), T->dWd_all + (size_t)off * ta.tx, (long long)b.cout * ta.tx});
      jobs.push_back({grad_of(m, b.prefix + ".dense_1.bias"), T->dbd_all + off, (long long)b.cout});
      T->cp_max = std::max<long long>(T->cp_max, (long long)b.cout * ta.tx);
      off += b.cout;
    };
    for (auto &b : m->enc) visit(b);
    for (auto &b : m->bott) visit(b);
    for (auto &b : m->dec) visit(b);
    T->n_cp_jobs = (int)jobs.size();
    if (dev_alloc(m, (void **)&T->d_cp_jobs, jobs.size() * sizeof(cm::CopyJob))) return 1;
    CM_HIP(hipMemcpyAsync(T->d_cp_jobs, jobs.data(), jobs.size() * sizeof(cm::CopyJob), hipMemcpyHostToDevice, st));
    CM_HIP(hipStreamSynchronize(st));
  }
  CM_HIP(cm::launch_copy_jobs(T->d_cp_jobs, T->n_cp_jobs, T->cp_max, st));
  // autocast: every gradient above carries the loss scale 2^k exactly (fp32 tensors); take it out once, so that the readers of the
  // flat buffer (cm_train_get_grad, the all-reduce, Adam, checkpoints) see unscaled gradients
  if (T->ls_k > 0) CM_HIP(cm::launch_scale_inplace(T->opt.g, (long long)T->opt.nfloats, ldexpf(1.f, -T->ls_k), st));
  return 0;
}

}  // namespace

extern "C" {

int cm_train_init(cm_model *m, float lr, float beta1, float beta2, float eps, float weight_decay, float dropout_rate) {
  CM_NOT_DIT(m, "cm_train_init");
  if (!m || !m->finalized) return fail("model not finalized");
  if (m->precision != CM_PRECISION_F32 && m->precision != CM_PRECISION_F32X)
    return fail("training runs on default-plan fp32 handles: the f16 operand copies of a reduced-precision handle are not re-packed after an "
                "update, and the relaxed plan is an inference plan");
  if (!(dropout_rate >= 0.f && dropout_rate < 1.f)) return fail("dropout rate %g outside [0,1)", dropout_rate);
  DevGuard g(m->device);
  if (!m->train) {
    m->train = new cm_train_state();
    if (train_setup(m)) return 1;
  }
  m->train->opt.hyper(lr, beta1, beta2, eps, weight_decay);
  m->train->dropout = dropout_rate;
  return 0;
}

int cm_train_set_sample_base(cm_model *m, int64_t sample_id_base) {
  if (!m || !m->train) return fail("cm_train_init has not been called");
  if (sample_id_base < 0) return fail("sample_id_base must be >= 0");
  m->train->sample_base = sample_id_base;
  return 0;
}

int cm_train_set_autocast(cm_model *m, int32_t mode, int32_t loss_scale_log2) {
  CM_NOT_DIT(m, "cm_train_set_autocast");
  if (!m) return fail("cm_train_set_autocast: null handle");
  if (mode != 0 && mode != 1) return fail("cm_train_set_autocast: mode %d: 0 = fp32 step, 1 = autocast", (int)mode);
  if (loss_scale_log2 > 24) return fail("cm_train_set_autocast: loss_scale_log2 %d above 24", (int)loss_scale_log2);
  if (!m->train) return fail("cm_train_set_autocast: cm_train_init has not been called");
  cm_train_state *T = m->train;
  DevGuard g(m->device);
  if (mode == 1) {
    if (!T->ac_ready) {
      // f16 siblings of the fp32 Winograd fragments: half their bytes, allocated once
      for (Op &op : m->ops)
        if (op.kind == OP_CONV && op.wino && op.d_wwino && op.wwino_floats > 0 &&
            dev_alloc(m, (void **)&op.d_wwino16t, (size_t)op.wwino_floats / 2 * sizeof(float))) return 1;
      for (auto &D : T->dg)
        if (D.wino && D.wwino && dev_alloc(m, (void **)&D.wwino16, (size_t)D.wwino_floats / 2 * sizeof(float))) return 1;
      // the job table of wino_pack_jobs_kernel with the f16 buffers as destinations: same order, same workgroup -> job map
      // (a model without Winograd layers -- narrow widths, odd grids -- has no such table and nothing to re-pack)
      if (!T->derived_wino.empty() && (!T->d_wjobs || !T->d_wblk2job)) return fail("cm_train_set_autocast: the Winograd re-pack table has not been built");
      std::map<const float *, float *> to16;
      for (Op &op : m->ops) if (op.d_wwino16t) to16[op.d_wwino] = op.d_wwino16t;
      for (auto &D : T->dg) if (D.wwino16) to16[D.wwino] = D.wwino16;
      std::vector<cm::WinoPackJob> jobs;
      long long blk = 0;
      for (auto &d : T->derived_wino) {
        cm::WinoPackJob j{};
        if (!to16.count(d.dst)) return fail("cm_train_set_autocast: a Winograd fragment set has no f16 sibling");
        j.dst = to16[d.dst]; j.idx27 = d.d_idx27; j.Co = d.Co; j.Ci = d.Ci; j.Ci_pad = d.Ci_pad; j.n = d.n; j.blk0 = blk;
        blk += (d.n + 255) / 256;
        jobs.push_back(j);
      }
      if (blk != T->wpack_blocks) return fail("cm_train_set_autocast: re-pack tables disagree");
      if (!jobs.empty()) {
        if (dev_alloc(m, (void **)&T->d_wjobs16, jobs.size() * sizeof(cm::WinoPackJob))) return 1;
        CM_HIP(hipMemcpy(T->d_wjobs16, jobs.data(), jobs.size() * sizeof(cm::WinoPackJob), hipMemcpyHostToDevice));
      }
      T->ac_ready = true;
    }
    // (the fp32 fragments are current: cm_train_init and every update re-derive them; the f16 ones only while the mode is on)
    if (repack_f16(m, m->stream)) return 1;
    CM_HIP(hipStreamSynchronize(m->stream));
  }
  T->autocast = mode; T->ls_req = mode ? (int)loss_scale_log2 : -1;
  if (!mode) T->ls_k = 0;
  m->train_autocast = mode == 1;
  return 0;
}

int cm_train_get_autocast(const cm_model *m, int32_t *mode, int32_t *loss_scale_log2) {
  CM_NOT_DIT(m, "cm_train_get_autocast");
  if (!m || !mode || !loss_scale_log2) return fail("cm_train_get_autocast: null argument");
  if (!m->train) return fail("cm_train_get_autocast: cm_train_init has not been called");
  const cm_train_state *T = m->train;
  *mode = T->autocast;
  *loss_scale_log2 = T->autocast ? autocast_scale_log2(m, T->ls_last_B > 0 ? T->ls_last_B : m->cfg.max_batch) : 0;
  return 0;
}

int cm_train_set_lr(cm_model *m, float lr) {
  if (!m || !m->train) return fail("cm_train_init has not been called");
  m->train->opt.lr = lr;
  return 0;
}

// Shared tail of a training step: train-mode forward on d_xt, MSE against d_target, backward, update.
static int train_step_core(cm_model *m, const float *d_xt, const float *d_past, const int64_t *d_t, const float *d_target,
                           const float *d_dropmask, uint64_t seed, float *h_loss, int32_t B, int32_t apply_update,
                           hipStream_t st) {
  cm_train_state *T = m->train;
  const cm_unet_config &c = m->cfg;
  const long long per = (long long)m->per_sample();
  if (make_plan(m, true, B, &m->plan)) return 1;
  T->ls_k = T->autocast ? autocast_scale_log2(m, B) : 0;
  if (T->autocast) T->ls_last_B = B;
  if (d_dropmask)
    CM_HIP(hipMemcpyAsync(m->dropmask, d_dropmask, (size_t)B * m->nproj * sizeof(float), hipMemcpyDeviceToDevice, st));
  else
    CM_HIP(cm::launch_dropout_mask(m->dropmask, B, m->nproj, T->dropout, seed, T->sample_base, T->opt.step, st));
  CM_HIP(hipMemcpyAsync(m->tbuf, d_t, (size_t)B * sizeof(long long), hipMemcpyDeviceToDevice, st));
  CM_HIP(cm::launch_time_mlp(m->d_time[0], m->d_time[1], m->d_time[2], m->d_time[3], m->d_time[4], m->d_time[5], m->d_time[6],
                             c.base_channels, c.base_channels * c.time_multiple, m->nproj, B, nullptr, T->train_temb,
                             m->tbuf, st));
  CM_HIP(cm::launch_assemble_input(d_past, d_xt, m->x8, B, c.in_channels, c.rows, c.cols, c.past_len, c.future_len, 3, st));
  m->use_train_temb = true;
  int rc = run_ops(m, m->plan, st);
  m->use_train_temb = false;
  if (!rc) {
    hipError_t e = cm::launch_extract_output(m->eps_cl, 8, T->pred, B, c.out_channels, c.rows, c.cols, c.past_len, c.future_len, st);
    if (e != hipSuccess) rc = fail("extract failed");
  }
  if (!rc) {
    hipError_t e = cm::launch_mse_loss(T->pred, d_target, (long long)B * per, m->mse_partial, m->mse_loss, st);
    if (e == hipSuccess) e = cm::launch_mse_grad(T->pred, d_target, m->act_by_name.at("final")->g, B, c.out_channels, c.rows, c.cols, c.past_len, c.future_len, st, ldexpf(1.f, T->ls_k));
    if (e != hipSuccess) rc = fail("loss kernels failed");
  }
  if (!rc) rc = backward_ops(m, B, st);
  if (rc) return 1;
  if (apply_update && (T->opt.apply(st) || repack_all(m, st))) return 1;
  CM_HIP(hipMemcpyAsync(h_loss, m->mse_loss, sizeof(float), hipMemcpyDeviceToHost, st));
  CM_HIP(hipStreamSynchronize(st));
  return 0;
}

// One training step on device buffers: x_t = q_sample(future, t, eps); eps_hat = UNet(x_t, t, past)
// with Dropout3d; loss = mse(eps_hat, eps); backward; optional Adam update + re-pack.
int cm_train_step(cm_model *m, const cm_schedule *s, const float *d_future, const float *d_past, const int64_t *d_t,
                  const float *d_eps, const float *d_dropmask, uint64_t seed, float *h_loss, int32_t B,
                  int32_t apply_update, void *stream) {
  CM_NOT_DIT(m, "cm_train_step");
  if (check_ready(m, B)) return 1;
  if (!m->train) return fail("cm_train_init has not been called");
  if (!s || !d_future || !d_past || !d_t || !h_loss) return fail("null argument");
  DevGuard g(m->device);
  hipStream_t st = stream ? (hipStream_t)stream : m->stream;
  cm_train_state *T = m->train;
  const long long per = (long long)m->per_sample();
  if (!d_eps) {
    // eps ~ N(0,1) from the device Philox stream: one substream per (training step, sample)
    // (the draw counter is the Philox step word, the global sample index its sample word)
    CM_HIP(cm::launch_randn(T->eps_dev, B, per, seed, T->sample_base, 0x40000000 + (int)(T->draws & 0x3fffffff), st));
    T->draws += 1;
    d_eps = T->eps_dev;
  }
  CM_HIP(cm::launch_q_sample(d_future, (const long long *)d_t, d_eps, s->d_sab, s->d_s1m, T->xt, B, per, st));
  return train_step_core(m, T->xt, d_past, d_t, d_eps, d_dropmask, seed, h_loss, B, apply_update, st);
}

int cm_train_step_xt(cm_model *m, const float *d_xt, const float *d_past, const int64_t *d_t, const float *d_target,
                     const float *d_dropmask, uint64_t seed, float *h_loss, int32_t B, int32_t apply_update, void *stream) {
  CM_NOT_DIT(m, "cm_train_step_xt");
  if (check_ready(m, B)) return 1;
  if (!m->train) return fail("cm_train_init has not been called");
  if (!d_xt || !d_past || !d_t || !d_target || !h_loss) return fail("null argument");
  DevGuard g(m->device);
  hipStream_t st = stream ? (hipStream_t)stream : m->stream;
  return train_step_core(m, d_xt, d_past, d_t, d_target, d_dropmask, seed, h_loss, B, apply_update, st);
}

int cm_train_get_grad(cm_model *m, const char *name, float *h_out, int64_t numel) {
  if (!m || !m->train) return fail("bad argument");
  DevGuard g(m->device);
  return m->train->opt.copy_out(m->params, m->train->opt.g, name, numel, h_out);
}

// Adam state of one tensor (torch.optim.Adam state_dict layout: 'exp_avg', 'exp_avg_sq'; 'step' from
// cm_train_opt_step) -- what utils/utils.py:140-147 stores under "opt".  which: 0 exp_avg, 1 exp_avg_sq, nothing else.
static int train_which(const char *what, int32_t which) {
  return which == 0 || which == 1 ? 0 : fail("%s: optimizer state %d: 0 = exp_avg, 1 = exp_avg_sq", what, which);
}
int cm_train_get_opt_state(cm_model *m, const char *name, int32_t which, float *h_out, int64_t numel) {
  if (train_which("cm_train_get_opt_state", which)) return 1;
  if (!m || !m->train) return fail("bad argument");
  DevGuard g(m->device);
  OptStore &S = m->train->opt;
  return S.copy_out(m->params, which ? S.v : S.m, name, numel, h_out);
}
int cm_train_set_opt_state(cm_model *m, const char *name, int32_t which, const float *h_in, int64_t numel) {
  if (train_which("cm_train_set_opt_state", which)) return 1;
  if (!m || !m->train) return fail("bad argument");
  DevGuard g(m->device);
  OptStore &S = m->train->opt;
  return S.copy_in(m->params, which ? S.v : S.m, name, numel, h_in);
}
int cm_train_opt_step(cm_model *m, int32_t *step, int32_t set) {
  if (!m || !m->train) return fail("bad argument");
  return m->train->opt.opt_step(step, set);
}

// Data-parallel training: the flat gradient buffer (state_dict order, fp32) for an all-reduce between
// cm_train_step(apply_update=0) and cm_train_apply.
int cm_train_flat_grads(cm_model *m, void **d_grads, int64_t *numel) {
  if (!m || !m->train) return fail("bad argument");
  return m->train->opt.flat_grads(d_grads, numel);
}
int cm_train_apply(cm_model *m, void *stream) {
  if (!m || !m->train) return fail("cm_train_init has not been called");
  DevGuard g(m->device);
  hipStream_t st = stream ? (hipStream_t)stream : m->stream;
  if (m->train->opt.apply(st) || repack_all(m, st)) return 1;
  CM_HIP(hipStreamSynchronize(st));
  return 0;
}

// Copy the master weights back into the host-side state_dict and rebuild the time-embedding
// table, so that cm_model_get_param / the sampling path see the trained weights.
int cm_train_sync(cm_model *m) {
  if (!m || !m->train) return fail("cm_train_init has not been called");
  DevGuard g(m->device);
  if (m->train->opt.pull_masters(m->params)) return 1;
  const cm_unet_config &c = m->cfg;
  CM_HIP(cm::launch_time_mlp(m->d_time[0], m->d_time[1], m->d_time[2], m->d_time[3], m->d_time[4], m->d_time[5], m->d_time[6],
                             c.base_channels, c.base_channels * c.time_multiple, m->nproj, TIME_ROWS, nullptr,
                             m->temb_table, nullptr, m->stream));
  CM_HIP(hipStreamSynchronize(m->stream));
  return refresh_h2(m);                             // (the sampling path's h2 fragments, here rather than inside its first call)
}

}  // extern "C"
