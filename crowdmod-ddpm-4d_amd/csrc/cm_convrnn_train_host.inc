// Training of the ConvRNN forecaster (convRNN.py:98-171: evaluate_loss, backward, torch.optim.Adam(amsgrad=True)), included
// by cm_convrnn_host.inc.  Kernels: cm_convrnn_train.hip; the forward is cm_convrnn.hip's conv kernel writing into a tape.
//
// Tape.  Layer i is applied A_i times per step: Ft * P for the encoder layers 0-5, Ft for the forecaster layers 6-12, and
// application a of a layer writes slot a of [A_i][B][h][w][C] buffers: the LeakyReLU output of a conv; r, r * h_prev, u and
// the candidate of a GRU cell; the four activated gates and tanh(c') of an LSTM cell.  The hidden state of level l is a tape
// of its own, H[l] = [Ft * (P + 1) + 1][B][h][w][hid] with slot 0 zero: cell step s of the level (the encoder cell at (t, p)
// is step t (P + 1) + p, the forecaster cell of t is step t (P + 1) + P) reads slot s and writes slot s + 1; likewise C[l].
//
// Backward, t = Ft - 1 .. 0, layers in reverse.  dH[l][2] is a ping-pong pair per level: when cell step s runs backward, `cur`
// holds the complete gradient of H[s + 1] and `prev` is first WRITTEN with the u * dh' term (zero for the LSTM), then receives
// += in this fixed order: the candidate path through r, the gates path, and -- once the layers in front of the cell run -- the
// data gradient of the conv that read H[s] (every tensor's readers are visited in the reverse of the forward order).
// Weight gradients: every application adds its tile sums to the split-K partials of its conv, in stream order; one reduce per
// conv at the end writes the reference layout through the index table of the packed layout.

struct CrnnTConv {
  int geo = 0;            // forward geometry (CRNN_GEO_*)
  int N = 0, Nr = 0;      // output channels; columns of its output-gradient buffer (N rounded up to 8)
  int cin = 0, cpad = 0;  // input channels (both sources), rounded up to 8
  float **fw = nullptr;   // the forward's packed weights (CrnnLayer::w0 / w1)
  size_t nf = 0, nb = 0, npart = 0;   // elements of the forward pack, the backward pack, one split of the partials
  unsigned *fidx = nullptr, *bidx = nullptr;
  float *bw = nullptr, *part = nullptr;
  int level_m = 0;        // level whose pixels are the rows of the weight gradient's K
};

struct CrnnTrain {
  OptStore opt;              // cm_opt_store.inc: no frozen tensor, with vmax (AMSGrad)
  CrnnTConv cv[13][2];
  float *tp[13][4] = {};     // tape buffers of a layer (see above)
  float *H[3] = {}, *Ct[3] = {};
  float *dH[3][2] = {}, *dC[3] = {}, *dx[3] = {}, *dcand[3] = {}, *dgate[3] = {};
  float *yhat = nullptr, *dY = nullptr;   // raw frames [B][4][HW][F]; d loss / d yhat [F][B][HW][8]
  double *lpart = nullptr, *lsums = nullptr, *lterms = nullptr;
  int dcur[3] = {0, 0, 0};
  int lastB = 0;
  // The split (data-parallel) step.  cm_convrnn_train_forward keeps its target frames in ytgt and its forcing mode in
  // split_tf; cm_convrnn_train_backward uploads the global sums from hsums (which outlives the call) to gsums.
  // m->tape_ready says that the tape, the window and ytgt are those of such a forward, with nothing run since.
  float *ytgt = nullptr;
  double *gsums = nullptr, hsums[6] = {};
  int split_tf = 0;
};

void crnn_free_train(CrnnTrain *t) { delete t; }

namespace {

// ---- backward weight layouts, from the forward's packed matrix Wf [N][9 * cpad] (values or indices) ----
// 3x3 stride 1: Wd[c][tap' * Nr + n] = Wf[n][(8 - tap') * cpad + c]: the same gather geometry reads dy at q + (tap' - centre),
// which the forward reached through tap 8 - tap'.  Columns n >= N stay 0.
template <class T>
std::vector<T> crnn_pack_d_s1(const std::vector<T> &wf, int N, int Nr, int cpad) {
  std::vector<T> out((size_t)cpad * 9 * Nr, T(0));
  for (int c = 0; c < cpad; ++c)
    for (int t = 0; t < 9; ++t)
      for (int n = 0; n < N; ++n) out[((size_t)c * 9 + t) * Nr + n] = wf[((size_t)n * 9 + (8 - t)) * cpad + c];
  return out;
}

// 3x3 stride 2: input pixel (2 qy + py, 2 qx + px) is read by output (qy + py - ty, qx + px - tx) through tap
// (1 - py + 2 ty, 1 - px + 2 tx), ty <= py, tx <= px: classes (py, px) of 1, 2, 2, 4 taps, one after the other, each
// [c][(ty * (1 + px) + tx) * N + n].
template <class T>
std::vector<T> crnn_pack_d_p3(const std::vector<T> &wf, int N, int C) {
  std::vector<T> out((size_t)9 * C * N, T(0));
  size_t base = 0;
  for (int cls = 0; cls < 4; ++cls) {
    const int py = cls >> 1, px = cls & 1, nt = (1 + py) * (1 + px);
    for (int c = 0; c < C; ++c)
      for (int tap = 0; tap < nt; ++tap)
        for (int n = 0; n < N; ++n) {
          const int ky = 1 - py + 2 * (tap / (1 + px)), kx = 1 - px + 2 * (tap % (1 + px));
          out[base + ((size_t)c * nt + tap) * N + n] = wf[((size_t)n * 9 + ky * 3 + kx) * C + c];
        }
    base += (size_t)nt * C * N;
  }
  return out;
}

// ConvTranspose2d 4x4 stride 2 pad 1, w [C][N][4][4]: dx[c](iy, ix) = sum dy[n](2 iy - 1 + ky, 2 ix - 1 + kx) w[c][n][ky][kx],
// a 16-tap stride-2 gather: Wd[c][(ky * 4 + kx) * N + n].  The weight gradient is produced in this layout as well.
template <class T>
std::vector<T> crnn_pack_d_g4(const T *w, int C, int N) {
  std::vector<T> out((size_t)C * 16 * N);
  for (int c = 0; c < C; ++c)
    for (int tap = 0; tap < 16; ++tap)
      for (int n = 0; n < N; ++n) out[((size_t)c * 16 + tap) * N + n] = w[((size_t)c * N + n) * 16 + tap];
  return out;
}

// Forward and backward packs of layer i: f[j], b[j] for conv j (1: the GRU candidate)
template <class T, class S>
void crnn_pack_train_t(const cm_convrnn *m, int i, S src, std::vector<T> f[2], std::vector<T> b[2]) {
  const CrnnLayer &l = m->L[i];
  crnn_pack_layer_t<T>(m, i, src, &f[0], &f[1]);
  b[1].clear();
  if (l.kind == CRNN_UP) { b[0] = crnn_pack_d_g4<T>(src(0), l.cin, l.cout); return; }
  if (l.kind == CRNN_DOWN) { b[0] = crnn_pack_d_p3<T>(f[0], l.cout, l.cin); return; }
  if (l.kind == CRNN_CONV) { b[0] = crnn_pack_d_s1<T>(f[0], l.cout, (l.cout + 7) / 8 * 8, (l.cin + 7) / 8 * 8); return; }
  const int hid = l.cout, cin = l.cin + hid, gru = m->cfg.cell == CM_CELL_GRU;
  b[0] = crnn_pack_d_s1<T>(f[0], (gru ? 2 : 4) * hid, (gru ? 2 : 4) * hid, cin);
  if (gru) b[1] = crnn_pack_d_s1<T>(f[1], hid, hid, cin);
}

int crnn_apps(const cm_convrnn *m, int i) { return m->cfg.future_len * (i < 6 ? m->cfg.past_len : 1); }
// split-K ranges of a weight gradient: about 256 rows each, at most 16; a function of B x pixels only, never of max_batch
int crnn_nsplit(long long rows) { return (int)std::min<long long>(16, std::max<long long>(1, (rows + 255) / 256)); }

int crnn_train_ready(const cm_convrnn *m, int B, bool need_train) {
  if (!m) return fail("null ConvRNN handle");
  if (m->precision != CM_PRECISION_F32)
    return fail("the f16 plan of a ConvRNN handle (cm_convrnn_set_precision(CM_PRECISION_F16)) is inference only: train and "
                "evaluate the loss on a CM_PRECISION_F32 handle");
  if (m->device < 0) return fail("host-only ConvRNN handle (device < 0) cannot train or evaluate a loss");
  if (!m->finalized) return fail("cm_convrnn_finalize has not been called");
  if (need_train && !m->train) return fail("cm_convrnn_train_init has not been called");
  if (B < 1 || B > m->cfg.max_batch) return fail("batch %d outside [1, max_batch=%d]", B, m->cfg.max_batch);
  return 0;
}

// Re-pack every forward and backward weight layout from the master weights
int crnn_train_repack(cm_convrnn *m, hipStream_t st) {
  CrnnTrain *T = m->train;
  for (int i = 0; i < 13; ++i)
    for (int j = 0; j < 2; ++j) {
      const CrnnTConv &v = T->cv[i][j];
      if (!v.nf) continue;
      CM_HIP(cm::launch_crnn_gather(T->opt.p, v.fidx, *v.fw, (long long)v.nf, st));
      CM_HIP(cm::launch_crnn_gather(T->opt.p, v.bidx, v.bw, (long long)v.nb, st));
    }
  return 0;
}

struct CrnnTapeRun {
  cm_convrnn *m; CrnnTrain *T; int B; hipStream_t st;
  long long pix[3];
  long long nH(int lv) const { return (long long)B * pix[lv] * m->hid[lv]; }
  float *slot(int i, int k, int app, long long per_pix) const { return T->tp[i][k] + (long long)app * B * pix[m->L[i].level] * per_pix; }
  float *Hs(int lv, int s) const { return T->H[lv] + (long long)s * nH(lv); }
  float *Cs(int lv, int s) const { return T->Ct[lv] + (long long)s * nH(lv); }
};

// forward of cell layer i, application `app`, step `s` of its level
int crnn_tape_cell(const CrnnTapeRun &R, int i, const float *x, int app, int s) {
  cm_convrnn *m = R.m;
  const CrnnLayer &l = m->L[i];
  const int lv = l.level, hid = l.cout;
  const float *hp = R.Hs(lv, s);
  float *hn = R.Hs(lv, s + 1);
  cm::CrnnConvArgs a = crnn_args(m, cm::CRNN_GEO_S1, 0, l.w0, R.B, lv, lv);
  a.x0 = x; a.bs0 = R.pix[lv] * l.cin; a.C0 = l.cin;
  a.x1 = hp; a.bs1 = R.pix[lv] * hid; a.C1 = hid;
  if (m->cfg.cell == CM_CELL_GRU) {
    float *rh = R.slot(i, 1, app, hid);
    a.epi = cm::CRNN_EPI_GRU_GATES; a.N = 2 * hid; a.y = rh; a.u = R.slot(i, 2, app, hid); a.hprev = hp; a.t0 = R.slot(i, 0, app, hid);
    CM_HIP(cm::launch_crnn_conv(a, R.st));
    a.epi = cm::CRNN_EPI_GRU_CAND; a.N = hid; a.W = l.w1; a.x1 = rh; a.y = hn; a.t0 = R.slot(i, 3, app, hid);
    CM_HIP(cm::launch_crnn_conv(a, R.st));
  } else {
    a.epi = cm::CRNN_EPI_LSTM; a.N = 4 * hid; a.y = hn; a.c = R.Cs(lv, s); a.cn = R.Cs(lv, s + 1);
    a.t0 = R.slot(i, 0, app, 4 * hid); a.t1 = R.slot(i, 1, app, hid);
    CM_HIP(cm::launch_crnn_conv(a, R.st));
  }
  return 0;
}

int crnn_tape_conv(const CrnnTapeRun &R, int i, const float *x, long long bs, int cx, int lin, int app) {
  const CrnnLayer &l = R.m->L[i];
  return crnn_conv(R.m, l, x, bs, cx, lin, R.slot(i, 0, app, l.cout), R.B, R.st);
}

// The forecast of crnn_run with every intermediate kept: raw frames into T->yhat
int crnn_tape_forward(const CrnnTapeRun &R, const float *d_past, const float *d_target, int tf) {
  cm_convrnn *m = R.m;
  CrnnTrain *T = R.T;
  const cm_convrnn_config &c = m->cfg;
  const int H = c.rows, W = c.cols, P = c.past_len, Ft = c.future_len, nslots = P + Ft, B = R.B;
  const long long HW = (long long)H * W, win_bs = (long long)nslots * HW * 8;
  hipStream_t st = R.st;
  for (int l = 0; l < 3; ++l) {
    CM_HIP(hipMemsetAsync(T->H[l], 0, (size_t)R.nH(l) * sizeof(float), st));
    if (T->Ct[l]) CM_HIP(hipMemsetAsync(T->Ct[l], 0, (size_t)R.nH(l) * sizeof(float), st));
  }
  CM_HIP(cm::launch_crnn_pack_frames(d_past, m->win, B, H, W, P, nslots, 0, st));
  if (tf) CM_HIP(cm::launch_crnn_pack_frames(d_target, m->win, B, H, W, Ft, nslots, P, st));
  const CrnnLayer *L = m->L;
  for (int t = 0; t < Ft; ++t) {
    for (int p = 0; p < P; ++p) {
      const int app = t * P + p, s = t * (P + 1) + p;
      if (crnn_tape_conv(R, 0, m->win + (long long)(t + p) * HW * 8, win_bs, 8, 2, app)) return 1;
      if (crnn_tape_cell(R, 1, R.slot(0, 0, app, L[0].cout), app, s)) return 1;
      if (crnn_tape_conv(R, 2, R.Hs(2, s + 1), R.pix[2] * m->hid[2], m->hid[2], 2, app)) return 1;
      if (crnn_tape_cell(R, 3, R.slot(2, 0, app, L[2].cout), app, s)) return 1;
      if (crnn_tape_conv(R, 4, R.Hs(1, s + 1), R.pix[1] * m->hid[1], m->hid[1], 1, app)) return 1;
      if (crnn_tape_cell(R, 5, R.slot(4, 0, app, L[4].cout), app, s)) return 1;
    }
    const int s = t * (P + 1) + P;
    if (crnn_tape_cell(R, 6, R.Hs(0, s), t, s)) return 1;
    if (crnn_tape_conv(R, 7, R.Hs(0, s + 1), R.pix[0] * m->hid[0], m->hid[0], 0, t)) return 1;
    if (crnn_tape_cell(R, 8, R.slot(7, 0, t, L[7].cout), t, s)) return 1;
    if (crnn_tape_conv(R, 9, R.Hs(1, s + 1), R.pix[1] * m->hid[1], m->hid[1], 1, t)) return 1;
    if (crnn_tape_cell(R, 10, R.slot(9, 0, t, L[9].cout), t, s)) return 1;
    if (crnn_tape_conv(R, 11, R.Hs(2, s + 1), R.pix[2] * m->hid[2], m->hid[2], 2, t)) return 1;
    cm::CrnnConvArgs a = crnn_args(m, cm::CRNN_GEO_S1, cm::CRNN_EPI_LAST, L[12].w0, B, 2, 2);
    a.x0 = R.slot(11, 0, t, L[11].cout); a.bs0 = HW * L[12].cin; a.C0 = L[12].cin; a.N = c.in_channels;
    a.out = T->yhat; a.Ft = Ft; a.t = t; a.exp_out = 0;
    a.win = tf ? nullptr : m->win + (long long)(P + t) * HW * 8; a.win_bs = win_bs;
    CM_HIP(cm::launch_crnn_conv(a, st));
  }
  T->lastB = B;
  return 0;
}

// Weight gradient of conv j of layer i: dy [B][pixels of the layer's output level][Nr] against the sources the forward read
int crnn_wgrad(const CrnnTapeRun &R, int i, int j, const float *dy, const float *x0, long long bs0, int C0, const float *x1, int lin) {
  const cm_convrnn *m = R.m;
  const CrnnLayer &l = m->L[i];
  const CrnnTConv &v = R.T->cv[i][j];
  cm::CrnnWgradArgs a{};
  a.B = R.B; a.part = v.part;
  if (l.kind == CRNN_UP) {   // rows: the input's pixels; gathered: the output gradient
    a.geo = cm::CRNN_BG_G4; a.R = x0; a.Nr = l.cin; a.Hm = m->lh[lin]; a.Wm = m->lw[lin];
    a.x0 = dy; a.bs0 = R.pix[l.level] * v.Nr; a.C0 = v.Nr; a.Hs = m->lh[l.level]; a.Ws = m->lw[l.level];
  } else {
    a.geo = l.kind == CRNN_DOWN ? cm::CRNN_BG_S2 : cm::CRNN_BG_S1; a.R = dy; a.Nr = v.Nr; a.Hm = m->lh[l.level]; a.Wm = m->lw[l.level];
    a.x0 = x0; a.bs0 = bs0; a.C0 = C0; a.Hs = m->lh[lin]; a.Ws = m->lw[lin];
    if (x1) { a.x1 = x1; a.C1 = l.cout; a.bs1 = R.pix[l.level] * l.cout; }
  }
  a.nsplit = crnn_nsplit((long long)R.B * a.Hm * a.Wm);
  CM_HIP(cm::launch_crnn_wgrad(a, R.st));
  return 0;
}

// Backward of cell layer i (application app, level step s): dH[lv][cur] is d h'.  Leaves d h_prev in dH[lv][prev] (and swaps),
// and the gradient of the cell's input in T->dx[lv], scaled by the LeakyReLU slope of `xmask` when the input is a conv's output.
int crnn_cell_bwd(const CrnnTapeRun &R, int i, const float *x, const float *xmask, int app, int s) {
  cm_convrnn *m = R.m;
  CrnnTrain *T = R.T;
  const CrnnLayer &l = m->L[i];
  const int lv = l.level, hid = l.cout;
  const long long n = R.nH(lv), bsx = R.pix[lv] * l.cin;
  float *dcur = T->dH[lv][T->dcur[lv]], *dprev = T->dH[lv][T->dcur[lv] ^ 1];
  const float *hp = R.Hs(lv, s);
  cm::CrnnDgradArgs d{};
  d.geo = cm::CRNN_BG_S1; d.B = R.B; d.Hs = d.Hd = m->lh[lv]; d.Ws = d.Wd_ = m->lw[lv]; d.C0 = l.cin; d.C1 = hid;
  d.d0 = T->dx[lv]; d.d1 = dprev;
  if (m->cfg.cell == CM_CELL_GRU) {
    const float *r = R.slot(i, 0, app, hid), *rh = R.slot(i, 1, app, hid), *u = R.slot(i, 2, app, hid), *cand = R.slot(i, 3, app, hid);
    CM_HIP(cm::launch_crnn_gru_bwd(dcur, u, cand, hp, dprev, T->dcand[lv], T->dgate[lv], n, hid, R.st));
    if (crnn_wgrad(R, i, 1, T->dcand[lv], x, bsx, l.cin, rh, lv)) return 1;
    d.dy = T->dcand[lv]; d.Cs = hid; d.Wd = T->cv[i][1].bw; d.acc0 = 0; d.acc1 = 1; d.gr = r; d.gh = hp; d.gdr = T->dgate[lv];
    CM_HIP(cm::launch_crnn_dgrad(d, R.st));
    if (crnn_wgrad(R, i, 0, T->dgate[lv], x, bsx, l.cin, hp, lv)) return 1;
    d.dy = T->dgate[lv]; d.Cs = 2 * hid; d.Wd = T->cv[i][0].bw; d.acc0 = 1; d.mask0 = xmask; d.gr = d.gh = nullptr; d.gdr = nullptr;
    CM_HIP(cm::launch_crnn_dgrad(d, R.st));
  } else {
    CM_HIP(cm::launch_crnn_lstm_bwd(dcur, R.slot(i, 0, app, 4 * hid), R.Cs(lv, s), R.slot(i, 1, app, hid), T->dC[lv], dprev, T->dgate[lv], n,
                                    hid, R.st));
    if (crnn_wgrad(R, i, 0, T->dgate[lv], x, bsx, l.cin, hp, lv)) return 1;
    d.dy = T->dgate[lv]; d.Cs = 4 * hid; d.Wd = T->cv[i][0].bw; d.acc0 = 0; d.acc1 = 1; d.mask0 = xmask;
    CM_HIP(cm::launch_crnn_dgrad(d, R.st));
  }
  T->dcur[lv] ^= 1;
  return 0;
}

// Backward of conv / down / up layer i whose output gradient (slope already applied) is dy: its weight gradient, and its data
// gradient added to `dst` (the gradient of the hidden state it read) or, with mask, written to it.
int crnn_conv_bwd(const CrnnTapeRun &R, int i, const float *dy, const float *x, int lin, float *dst, const float *mask) {
  cm_convrnn *m = R.m;
  const CrnnLayer &l = m->L[i];
  const CrnnTConv &v = R.T->cv[i][0];
  if (crnn_wgrad(R, i, 0, dy, x, R.pix[lin] * v.cpad, v.cpad, nullptr, lin)) return 1;
  if (!dst) return 0;
  cm::CrnnDgradArgs d{};
  d.geo = l.kind == CRNN_UP ? cm::CRNN_BG_G4 : l.kind == CRNN_DOWN ? cm::CRNN_BG_P3 : cm::CRNN_BG_S1;
  d.dy = dy; d.Cs = v.Nr; d.Hs = m->lh[l.level]; d.Ws = m->lw[l.level]; d.Wd = v.bw;
  d.B = R.B; d.Hd = m->lh[lin]; d.Wd_ = m->lw[lin]; d.C0 = v.cpad; d.d0 = dst; d.acc0 = mask ? 0 : 1; d.mask0 = mask;
  CM_HIP(cm::launch_crnn_dgrad(d, R.st));
  return 0;
}

int crnn_train_backward(const CrnnTapeRun &R, int tf) {
  cm_convrnn *m = R.m;
  CrnnTrain *T = R.T;
  const cm_convrnn_config &c = m->cfg;
  const int P = c.past_len, Ft = c.future_len, nslots = P + Ft, B = R.B;
  const long long HW = (long long)c.rows * c.cols, win_bs = (long long)nslots * HW * 8;
  const CrnnLayer *L = m->L;
  hipStream_t st = R.st;
  for (int i = 0; i < 13; ++i)
    for (int j = 0; j < 2; ++j) {
      const CrnnTConv &v = T->cv[i][j];
      if (v.nf) CM_HIP(hipMemsetAsync(v.part, 0, (size_t)crnn_nsplit((long long)B * R.pix[v.level_m]) * v.npart * sizeof(float), st));
    }
  for (int l = 0; l < 3; ++l) {
    CM_HIP(hipMemsetAsync(T->dH[l][0], 0, (size_t)R.nH(l) * sizeof(float), st));
    if (T->dC[l]) CM_HIP(hipMemsetAsync(T->dC[l], 0, (size_t)R.nH(l) * sizeof(float), st));
    T->dcur[l] = 0;
  }
  auto cur = [&](int lv) { return T->dH[lv][T->dcur[lv]]; };
  for (int t = Ft - 1; t >= 0; --t) {
    const int s = t * (P + 1) + P;
    const float *dy12 = T->dY + (long long)t * B * HW * 8;
    const float *a5 = R.slot(11, 0, t, L[11].cout);
    if (crnn_conv_bwd(R, 12, dy12, a5, 2, T->dx[2], a5)) return 1;
    if (crnn_conv_bwd(R, 11, T->dx[2], R.Hs(2, s + 1), 2, cur(2), nullptr)) return 1;
    const float *a4 = R.slot(9, 0, t, L[9].cout);
    if (crnn_cell_bwd(R, 10, a4, a4, t, s)) return 1;
    if (crnn_conv_bwd(R, 9, T->dx[2], R.Hs(1, s + 1), 1, cur(1), nullptr)) return 1;
    const float *a3 = R.slot(7, 0, t, L[7].cout);
    if (crnn_cell_bwd(R, 8, a3, a3, t, s)) return 1;
    if (crnn_conv_bwd(R, 7, T->dx[1], R.Hs(0, s + 1), 0, cur(0), nullptr)) return 1;
    // frnn1 reads the encoder's last h both as its input and as h_prev: the input's gradient joins d h_prev last
    if (crnn_cell_bwd(R, 6, R.Hs(0, s), nullptr, t, s)) return 1;
    CM_HIP(cm::launch_crnn_add(cur(0), T->dx[0], R.nH(0), st));
    for (int p = P - 1; p >= 0; --p) {
      const int app = t * P + p, se = t * (P + 1) + p;
      const float *a2 = R.slot(4, 0, app, L[4].cout), *a1 = R.slot(2, 0, app, L[2].cout), *a0 = R.slot(0, 0, app, L[0].cout);
      if (crnn_cell_bwd(R, 5, a2, a2, app, se)) return 1;
      if (crnn_conv_bwd(R, 4, T->dx[0], R.Hs(1, se + 1), 1, cur(1), nullptr)) return 1;
      if (crnn_cell_bwd(R, 3, a1, a1, app, se)) return 1;
      if (crnn_conv_bwd(R, 2, T->dx[1], R.Hs(2, se + 1), 2, cur(2), nullptr)) return 1;
      if (crnn_cell_bwd(R, 1, a0, a0, app, se)) return 1;
      // the first conv: its weight gradient over window slot t + p; a slot the model filled itself (no teacher forcing)
      // hands its data gradient back to the frame it came from, through the exp on channels 0 and 3
      const CrnnTConv &v = T->cv[0][0];
      cm::CrnnWgradArgs w{};
      w.geo = cm::CRNN_BG_S1; w.R = T->dx[2]; w.Nr = v.Nr; w.B = B; w.Hm = w.Hs = c.rows; w.Wm = w.Ws = c.cols;
      w.x0 = m->win + (long long)(t + p) * HW * 8; w.bs0 = win_bs; w.C0 = 8; w.nsplit = crnn_nsplit((long long)B * HW); w.part = v.part;
      CM_HIP(cm::launch_crnn_wgrad(w, st));
      if (!tf && t + p >= P) {
        cm::CrnnDgradArgs d{};
        d.geo = cm::CRNN_BG_S1; d.dy = T->dx[2]; d.Cs = v.Nr; d.Hs = d.Hd = c.rows; d.Ws = d.Wd_ = c.cols; d.Wd = v.bw; d.B = B; d.C0 = 8;
        d.d0 = T->dY + (long long)(t + p - P) * B * HW * 8; d.fb_exp = m->win + (long long)(t + p) * HW * 8; d.fb_bs = win_bs; d.fb_C = 4;
        CM_HIP(cm::launch_crnn_dgrad(d, st));
      }
    }
  }
  for (int i = 0; i < 13; ++i)
    for (int j = 0; j < 2; ++j) {
      const CrnnTConv &v = T->cv[i][j];
      if (!v.nf) continue;
      const bool up = L[i].kind == CRNN_UP;
      CM_HIP(cm::launch_crnn_wgrad_reduce(v.part, crnn_nsplit((long long)B * R.pix[v.level_m]), (long long)v.npart, (long long)(up ? v.nb : v.nf),
                                          up ? v.bidx : v.fidx, T->opt.g, st));
    }
  return 0;
}

CrnnTapeRun crnn_tape_of(cm_convrnn *m, int B, hipStream_t st) {
  return CrnnTapeRun{m, m->train, B, st, {(long long)m->lh[0] * m->lw[0], (long long)m->lh[1] * m->lw[1], (long long)m->lh[2] * m->lw[2]}};
}

// forward (+ loss) (+ backward) (+ update); the four terms come back after one synchronisation at the end
int crnn_train_run(cm_convrnn *m, const float *d_past, const float *d_target, int tf, double loss_eps, double alpha, int backward,
                   int apply_update, double h_terms[4], int B, hipStream_t st) {
  CrnnTrain *T = m->train;
  const cm_convrnn_config &c = m->cfg;
  CrnnTapeRun R = crnn_tape_of(m, B, st);
  m->tape_ready = false;
  if (crnn_tape_forward(R, d_past, d_target, tf)) return 1;
  const int HW = c.rows * c.cols;
  CM_HIP(cm::launch_crnn_loss(T->yhat, d_target, B, HW, c.future_len, loss_eps, T->lpart, T->lsums, T->lterms, st));
  if (backward) {
    CM_HIP(cm::launch_crnn_loss_grad(T->yhat, d_target, B, HW, c.future_len, loss_eps, alpha, T->lsums,
                                     (double)((long long)B * HW * c.future_len), T->dY, st));
    if (crnn_train_backward(R, tf)) return 1;
    if (apply_update && (T->opt.apply(st) || crnn_train_repack(m, st))) return 1;
  }
  if (h_terms) {
    CM_HIP(hipMemcpyAsync(h_terms, T->lterms, 4 * sizeof(double), hipMemcpyDeviceToHost, st));
    CM_HIP(hipStreamSynchronize(st));
  }
  return 0;
}

// The first half of a split step, and its validation form: the tape forward and the loss sums.  h_sums[0..4] are the five
// sums of this call's samples, h_sums[5] their element count B HW F, after one synchronisation.  With `keep` the target
// frames are copied to the handle and the tape is marked as waiting for crnn_split_backward.
int crnn_forward_sums(cm_convrnn *m, const float *d_past, const float *d_target, int tf, bool keep, double h_sums[6], int B, hipStream_t st) {
  CrnnTrain *T = m->train;
  const cm_convrnn_config &c = m->cfg;
  const int HW = c.rows * c.cols;
  const long long n = (long long)B * HW * c.future_len;
  m->tape_ready = false;
  if (crnn_tape_forward(crnn_tape_of(m, B, st), d_past, d_target, tf)) return 1;
  CM_HIP(cm::launch_crnn_loss(T->yhat, d_target, B, HW, c.future_len, 0.0, T->lpart, T->lsums, nullptr, st));
  if (keep) CM_HIP(hipMemcpyAsync(T->ytgt, d_target, (size_t)n * 4 * sizeof(float), hipMemcpyDeviceToDevice, st));
  CM_HIP(hipMemcpyAsync(h_sums, T->lsums, 5 * sizeof(double), hipMemcpyDeviceToHost, st));
  CM_HIP(hipStreamSynchronize(st));
  h_sums[5] = (double)n;
  T->split_tf = tf;
  m->tape_ready = keep;
  return 0;
}

// The second half: the four terms and d loss / d yhat from the GLOBAL sums (this rank's elements, the denominators of all
// ranks), then the backward over the tape crnn_forward_sums left.  The gradient is this rank's share of the global
// objective's: the shares are summed over ranks, not averaged.
int crnn_split_backward(cm_convrnn *m, const double g[6], double loss_eps, double alpha, double h_terms[4], hipStream_t st) {
  CrnnTrain *T = m->train;
  const cm_convrnn_config &c = m->cfg;
  const int B = T->lastB, HW = c.rows * c.cols;
  m->tape_ready = false;
  std::copy(g, g + 6, T->hsums);
  CM_HIP(hipMemcpyAsync(T->gsums, T->hsums, 6 * sizeof(double), hipMemcpyHostToDevice, st));
  CM_HIP(cm::launch_crnn_loss_terms(T->gsums, loss_eps, T->lterms, st));
  CM_HIP(cm::launch_crnn_loss_grad(T->yhat, T->ytgt, B, HW, c.future_len, loss_eps, alpha, T->gsums, g[5], T->dY, st));
  if (crnn_train_backward(crnn_tape_of(m, B, st), T->split_tf)) return 1;
  if (h_terms) {
    CM_HIP(hipMemcpyAsync(h_terms, T->lterms, 4 * sizeof(double), hipMemcpyDeviceToHost, st));
    CM_HIP(hipStreamSynchronize(st));
  }
  return 0;
}

int crnn_opt_buffer(OptStore &S, int which, float **buf) {
  *buf = which == 0 ? S.m : which == 1 ? S.v : which == 2 ? S.vmax : nullptr;
  return *buf ? 0 : fail("optimizer state %d: 0 = exp_avg, 1 = exp_avg_sq, 2 = max_exp_avg_sq", which);
}

}  // namespace

extern "C" {

int cm_convrnn_train_init(cm_convrnn *m, float lr, float beta1, float beta2, float eps, float weight_decay) {
  if (!m) return fail("null ConvRNN handle");
  if (m->precision != CM_PRECISION_F32)
    return fail("the f16 plan of a ConvRNN handle (cm_convrnn_set_precision(CM_PRECISION_F16)) is inference only: train and "
                "evaluate the loss on a CM_PRECISION_F32 handle");
  if (m->device < 0) return fail("cm_convrnn_train_init: host-only ConvRNN handle (device < 0) cannot train");
  if (!m->finalized) return fail("cm_convrnn_train_init: cm_convrnn_finalize has not been called");
  if (m->train) return fail("cm_convrnn_train_init has already been called on this handle");
  if (!(lr >= 0.f) || !(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f) || !(eps >= 0.f) || !(weight_decay >= 0.f))
    return fail("cm_convrnn_train_init: lr, eps, weight_decay must be >= 0 and betas in [0, 1)");
  DevGuard g(m->device);
  const cm_convrnn_config &c = m->cfg;
  auto T = std::make_unique<CrnnTrain>();
  T->opt.hyper(lr, beta1, beta2, eps, weight_decay);
  const size_t nfloats = opt_layout(m->params, {}).nfloats;
  if (nfloats >= 0xffffffffULL) return fail("cm_convrnn_train_init: %zu weights exceed the 32-bit index tables", nfloats);
  size_t bytes = 0;
  auto alloc = [&](float **p, size_t n) {
    n = std::max<size_t>(n, 8);
    bytes += n * sizeof(float);
    if (hipMalloc((void **)p, n * sizeof(float)) != hipSuccess)
      return fail("cm_convrnn_train_init: device allocation failed after %zu bytes (weights, optimizer state and tape for max_batch %d)", bytes,
                  c.max_batch);
    m->allocs.push_back(*p);
    return 0;
  };
  if (T->opt.init(m->params, {}, true, alloc)) return 1;

  const size_t MB = (size_t)c.max_batch;
  const bool gru = c.cell == CM_CELL_GRU;
  size_t pix[3];
  for (int l = 0; l < 3; ++l) pix[l] = (size_t)m->lh[l] * m->lw[l];
  std::vector<unsigned> ids(nfloats);
  for (size_t k = 0; k < ids.size(); ++k) ids[k] = (unsigned)(k + 1);
  std::vector<unsigned> fi[2], bi[2];
  std::vector<float> fv[2], bv[2];
  for (int i = 0; i < 13; ++i) {
    const CrnnLayer &l = m->L[i];
    const Param *pp = &m->params[l.p0];
    const size_t *po = &T->opt.off[l.p0];
    crnn_pack_train_t<unsigned>(m, i, [&](int j) { return ids.data() + po[j]; }, fi, bi);
    crnn_pack_train_t<float>(m, i, [&](int j) { return pp[j].host.data(); }, fv, bv);
    for (int j = 0; j < 2; ++j) {
      if (fi[j].empty()) continue;
      CrnnTConv &v = T->cv[i][j];
      const bool cell = l.kind == CRNN_CELL;
      v.geo = l.kind == CRNN_UP ? cm::CRNN_GEO_T4 : l.kind == CRNN_DOWN ? cm::CRNN_GEO_S2 : cm::CRNN_GEO_S1;
      v.N = cell ? (j ? 1 : gru ? 2 : 4) * l.cout : l.cout;
      v.Nr = (v.N + 7) / 8 * 8;
      v.cin = cell ? l.cin + l.cout : l.cin;
      v.cpad = (v.cin + 7) / 8 * 8;
      v.fw = j ? &m->L[i].w1 : &m->L[i].w0;
      v.nf = fi[j].size(); v.nb = bi[j].size();
      // rows of the weight gradient's K: the output pixels, or the input pixels of the transposed conv
      v.level_m = l.kind == CRNN_UP ? l.level - 1 : l.level;
      v.npart = l.kind == CRNN_UP ? v.nb : (size_t)v.Nr * 9 * v.cpad;
      if (alloc((float **)&v.fidx, v.nf) || alloc((float **)&v.bidx, v.nb) || alloc(&v.bw, v.nb) ||
          alloc(&v.part, (size_t)crnn_nsplit((long long)(MB * pix[v.level_m])) * v.npart))
        return 1;
      CM_HIP(hipMemcpy(v.fidx, fi[j].data(), v.nf * sizeof(unsigned), hipMemcpyHostToDevice));
      CM_HIP(hipMemcpy(v.bidx, bi[j].data(), v.nb * sizeof(unsigned), hipMemcpyHostToDevice));
      CM_HIP(hipMemcpy(v.bw, bv[j].data(), v.nb * sizeof(float), hipMemcpyHostToDevice));
    }
    // tape
    const size_t per = MB * pix[l.level] * crnn_apps(m, i), hid = (size_t)l.cout;
    if (l.kind != CRNN_CELL) {
      if (i < 12 && alloc(&T->tp[i][0], per * hid)) return 1;
    } else if (gru) {
      for (int k = 0; k < 4; ++k)
        if (alloc(&T->tp[i][k], per * hid)) return 1;
    } else {
      if (alloc(&T->tp[i][0], per * 4 * hid) || alloc(&T->tp[i][1], per * hid)) return 1;
    }
  }
  const size_t steps = (size_t)c.future_len * (c.past_len + 1) + 1;
  const size_t xch[3] = {(size_t)std::max(c.enc_hidden[4], c.forc_hidden[0]), (size_t)std::max(c.enc_hidden[2], c.forc_hidden[2]),
                         (size_t)std::max(std::max(c.enc_hidden[0], c.forc_hidden[4]), c.forc_hidden[6])};
  for (int l = 0; l < 3; ++l) {
    const size_t n = MB * pix[l] * m->hid[l];
    if (alloc(&T->H[l], steps * n) || alloc(&T->dH[l][0], n) || alloc(&T->dH[l][1], n) || alloc(&T->dcand[l], n) ||
        alloc(&T->dgate[l], (gru ? 2 : 4) * n) || alloc(&T->dx[l], MB * pix[l] * xch[l]))
      return 1;
    if (!gru && (alloc(&T->Ct[l], steps * n) || alloc(&T->dC[l], n))) return 1;
  }
  const size_t HW = pix[2], Ft = (size_t)c.future_len;
  if (alloc(&T->yhat, MB * 4 * HW * Ft) || alloc(&T->dY, Ft * MB * HW * 8)) return 1;
  const size_t nblk = (MB * HW * Ft + 255) / 256;
  if (alloc((float **)&T->lpart, 2 * 5 * nblk) || alloc((float **)&T->lsums, 2 * 5) || alloc((float **)&T->lterms, 2 * 4)) return 1;
  if (alloc(&T->ytgt, MB * 4 * HW * Ft) || alloc((float **)&T->gsums, 2 * 6)) return 1;
  m->train = T.release();
  return 0;
}

int cm_convrnn_loss(cm_convrnn *m, const float *d_past, const float *d_target, int32_t teacher_forcing, double loss_eps, double h_terms[4],
                    int32_t B, void *stream) {
  if (crnn_train_ready(m, B, true)) return 1;
  if (!d_past || !d_target || !h_terms) return fail("null argument");
  DevGuard g(m->device);
  return crnn_train_run(m, d_past, d_target, teacher_forcing != 0, loss_eps, 1.0, 0, 0, h_terms, B, stream ? (hipStream_t)stream : m->stream);
}

int cm_convrnn_train_step(cm_convrnn *m, const float *d_past, const float *d_target, int32_t teacher_forcing, double loss_eps, double alpha,
                          double h_terms[4], int32_t B, int32_t apply_update, void *stream) {
  if (crnn_train_ready(m, B, true)) return 1;
  if (!d_past || !d_target) return fail("null argument");
  DevGuard g(m->device);
  return crnn_train_run(m, d_past, d_target, teacher_forcing != 0, loss_eps, alpha, 1, apply_update != 0, h_terms, B,
                        stream ? (hipStream_t)stream : m->stream);
}

int cm_convrnn_train_forward(cm_convrnn *m, const float *d_past, const float *d_target, int32_t teacher_forcing, int32_t B, void *stream,
                             double h_sums[6]) {
  if (crnn_train_ready(m, B, true)) return 1;
  if (!d_past || !d_target || !h_sums) return fail("null argument");
  DevGuard g(m->device);
  return crnn_forward_sums(m, d_past, d_target, teacher_forcing != 0, true, h_sums, B, stream ? (hipStream_t)stream : m->stream);
}

int cm_convrnn_loss_sums(cm_convrnn *m, const float *d_past, const float *d_target, int32_t teacher_forcing, int32_t B, void *stream,
                         double h_sums[6]) {
  if (crnn_train_ready(m, B, true)) return 1;
  if (!d_past || !d_target || !h_sums) return fail("null argument");
  DevGuard g(m->device);
  return crnn_forward_sums(m, d_past, d_target, teacher_forcing != 0, false, h_sums, B, stream ? (hipStream_t)stream : m->stream);
}

int cm_convrnn_train_backward(cm_convrnn *m, const double h_global_sums[6], double loss_eps, double alpha, double h_terms[4], void *stream) {
  if (crnn_train_ready(m, 1, true)) return 1;
  if (!h_global_sums) return fail("null argument");
  if (!m->tape_ready)
    return fail("cm_convrnn_train_backward: no cm_convrnn_train_forward is waiting on this handle (it must come directly before)");
  const double own = (double)m->train->lastB * m->cfg.rows * m->cfg.cols * m->cfg.future_len;
  // the three counts are sums of ones: never NaN, whatever the loss sums are (a diverged run keeps its NaN terms)
  if (!(h_global_sums[2] >= 0) || !(h_global_sums[4] >= 0) || !(h_global_sums[5] >= own) || std::isinf(h_global_sums[5]))
    return fail("cm_convrnn_train_backward: global counts (%g occupied, %g empty, %g elements) cannot contain this handle's %g elements",
                h_global_sums[2], h_global_sums[4], h_global_sums[5], own);
  DevGuard g(m->device);
  return crnn_split_backward(m, h_global_sums, loss_eps, alpha, h_terms, stream ? (hipStream_t)stream : m->stream);
}

int cm_convrnn_train_flat_grads(cm_convrnn *m, float **d_ptr, int64_t *numel) {
  if (crnn_train_ready(m, 1, true)) return 1;
  return m->train->opt.flat_grads((void **)d_ptr, numel);
}

int cm_convrnn_loss_terms_from_sums(const double sums[6], double eps, double terms[4]) {
  if (!sums || !terms) return fail("null argument");
  if (!(sums[5] >= 1)) return fail("cm_convrnn_loss_terms_from_sums: element count %g < 1", sums[5]);
  cm::crnn_loss_terms(sums, sums[5], eps, terms);
  return 0;
}

int cm_convrnn_train_apply(cm_convrnn *m, void *stream) {
  if (crnn_train_ready(m, 1, true)) return 1;
  m->tape_ready = false;   // the tape is of the weights before the update
  DevGuard g(m->device);
  hipStream_t st = stream ? (hipStream_t)stream : m->stream;
  return m->train->opt.apply(st) || crnn_train_repack(m, st);
}

int cm_convrnn_train_set_lr(cm_convrnn *m, float lr) {
  if (crnn_train_ready(m, 1, true)) return 1;
  if (!(lr >= 0.f)) return fail("lr must be >= 0");
  m->train->opt.lr = lr;
  return 0;
}

int cm_convrnn_train_get_forecast(cm_convrnn *m, float *h_out, int64_t numel) {
  if (crnn_train_ready(m, 1, true)) return 1;
  if (!h_out) return fail("null argument");
  CrnnTrain *T = m->train;
  const int64_t n = (int64_t)T->lastB * 4 * m->cfg.rows * m->cfg.cols * m->cfg.future_len;
  if (T->lastB < 1) return fail("no training forward has run on this handle");
  if (numel != n) return fail("the last training forward left %lld elements, got %lld", (long long)n, (long long)numel);
  DevGuard g(m->device);
  CM_HIP(hipDeviceSynchronize());
  CM_HIP(hipMemcpy(h_out, T->yhat, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}

int cm_convrnn_train_get_grad(cm_convrnn *m, const char *name, float *h_data, int64_t numel) {
  if (crnn_train_ready(m, 1, true)) return 1;
  DevGuard g(m->device);
  return m->train->opt.copy_out(m->params, m->train->opt.g, name, numel, h_data);
}

int cm_convrnn_train_get_opt_state(cm_convrnn *m, const char *name, int32_t which, float *h_data, int64_t numel) {
  float *buf = nullptr;
  if (crnn_train_ready(m, 1, true) || crnn_opt_buffer(m->train->opt, which, &buf)) return 1;
  DevGuard g(m->device);
  return m->train->opt.copy_out(m->params, buf, name, numel, h_data);
}

int cm_convrnn_train_set_opt_state(cm_convrnn *m, const char *name, int32_t which, const float *h_data, int64_t numel) {
  float *buf = nullptr;
  if (crnn_train_ready(m, 1, true) || crnn_opt_buffer(m->train->opt, which, &buf)) return 1;
  DevGuard g(m->device);
  return m->train->opt.copy_in(m->params, buf, name, numel, h_data);
}

int cm_convrnn_train_opt_step(cm_convrnn *m, int32_t *step, int32_t set) {
  if (crnn_train_ready(m, 1, true)) return 1;
  return m->train->opt.opt_step(step, set);
}

int cm_convrnn_train_sync(cm_convrnn *m) {
  if (crnn_train_ready(m, 1, true)) return 1;
  DevGuard g(m->device);
  if (m->train->opt.pull_masters(m->params)) return 1;
  if (crnn_train_repack(m, m->stream)) return 1;
  CM_HIP(hipStreamSynchronize(m->stream));
  return 0;
}

}  // extern "C"
