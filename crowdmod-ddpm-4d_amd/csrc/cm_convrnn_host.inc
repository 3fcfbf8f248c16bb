// Host plan of the ConvRNN forecaster (models/convRNN/forecaster.py, encoder.py; arch "ConvRNN"), included by cm_model.cpp.
// The forecaster has no timestep and no sampler, so it is a handle of its own (cm_convrnn), not a cm_model.  Kernels:
// cm_convrnn.hip.  One cm_convrnn_forecast call enqueues every launch of all future_len steps on one stream: no host
// synchronisation and no allocation in between.
//
// Layers, in state_dict order (encoder.encoder_cell_list.0-5, forecaster_cell_list.0-6):
//   enc 0 conv 4 -> E0 | 1 cell(E0, E1) on hs[2] | 2 down E1 -> E2 | 3 cell(E1, E3) on hs[1] | 4 down E3 -> E4 | 5 cell(E3, E5) on hs[0]
//   forc 0 cell(F0, F1) on hs[0] | 1 up F1 -> F2 | 2 cell(F2, F3) on hs[1] | 3 up F3 -> F4 | 4 cell(F4, F5) on hs[2] | 5 conv F5 -> F6 | 6 conv F6 -> 4
// hs[l]: level l hidden state, 0 = quarter, 1 = half, 2 = full resolution, shared by encoder and forecaster.
// The observation window is not slid: frame p of step t's window is slot t + p of a [B][P + Ft][H][W][8] buffer, and the
// frame a step appends (target[..., t] under teacher forcing, else the prediction with exp on channels 0 and 3) is slot P + t.

enum CrnnKind { CRNN_CONV = 0, CRNN_DOWN = 1, CRNN_UP = 2, CRNN_CELL = 3 };
struct CrnnLayer {
  CrnnKind kind; int cin, cout, level;   // CRNN_CELL: cin = the declared input_dim, cout = hidden_dim, level = its hidden state
  int p0 = 0;                            // index of its first state_dict tensor
  float *w0 = nullptr, *w1 = nullptr;    // packed device weights (GRU: gates, candidate)
  _Float16 *h0 = nullptr, *h1 = nullptr; // f16 plan, layers 1-11: the same matrices rounded once to f16, instead of w0 / w1
};

struct cm_convrnn {
  cm_convrnn_config cfg{};
  int device = -1;
  int precision = CM_PRECISION_F32;      // cm_convrnn_set_precision: CM_PRECISION_F32 or CM_PRECISION_F16
  bool finalized = false;
  int lastB = 0;
  hipStream_t stream = nullptr;
  std::vector<Param> params;
  CrnnLayer L[13];
  int hid[3] = {0, 0, 0}, lh[3] = {0, 0, 0}, lw[3] = {0, 0, 0};   // per level: hidden channels, rows, cols
  float *win = nullptr, *act[6] = {}, *scr = nullptr, *u = nullptr, *h[3][2] = {}, *c[3] = {};
  float *st_past = nullptr, *st_tgt = nullptr, *st_out = nullptr;   // staging of the host-buffer entry point
  int cur[3] = {0, 0, 0};
  struct CrnnTrain *train = nullptr;   // cm_convrnn_train_host.inc
  bool tape_ready = false;             // a cm_convrnn_train_forward is waiting for its backward; any other run clears it
  std::vector<void *> allocs;
};
void crnn_free_train(CrnnTrain *t);

namespace {

const char *const CRNN_PREFIX[2] = {"encoder.encoder_cell_list.", "forecaster_cell_list."};

void crnn_build(cm_convrnn *m) {
  const cm_convrnn_config &c = m->cfg;
  const int32_t *E = c.enc_hidden, *F = c.forc_hidden;
  const CrnnLayer layers[13] = {
      {CRNN_CONV, c.in_channels, E[0], 2}, {CRNN_CELL, E[0], E[1], 2}, {CRNN_DOWN, E[1], E[2], 1}, {CRNN_CELL, E[1], E[3], 1},
      {CRNN_DOWN, E[3], E[4], 0},          {CRNN_CELL, E[3], E[5], 0},
      {CRNN_CELL, F[0], F[1], 0},          {CRNN_UP, F[1], F[2], 1},   {CRNN_CELL, F[2], F[3], 1},   {CRNN_UP, F[3], F[4], 2},
      {CRNN_CELL, F[4], F[5], 2},          {CRNN_CONV, F[5], F[6], 2}, {CRNN_CONV, F[6], c.in_channels, 2}};
  for (int i = 0; i < 13; ++i) {
    CrnnLayer &l = m->L[i];
    l = layers[i];
    l.p0 = (int)m->params.size();
    const std::string base = std::string(CRNN_PREFIX[i >= 6]) + std::to_string(i >= 6 ? i - 6 : i);
    auto add = [&](const std::string &suffix, std::vector<int64_t> shape) {
      Param p;
      p.name = base + suffix;
      p.shape = std::move(shape);
      p.host.assign((size_t)p.numel(), 0.f);
      m->params.push_back(std::move(p));
    };
    if (l.kind == CRNN_CELL && c.cell == CM_CELL_GRU) {
      for (const char *g : {".reset_gate.weight", ".update_gate.weight", ".conv_cand.weight"}) add(g, {l.cout, l.cin + l.cout, 3, 3});
    } else if (l.kind == CRNN_CELL) {
      add(".conv.weight", {4 * (int64_t)l.cout, l.cin + l.cout, 3, 3});
    } else if (l.kind == CRNN_UP) {
      add(".weight", {l.cin, l.cout, 4, 4});
    } else {
      add(".weight", {l.cout, l.cin, 3, 3});
    }
  }
  m->hid[0] = E[5]; m->hid[1] = E[3]; m->hid[2] = E[1];
  for (int l = 0; l < 3; ++l) { m->lh[l] = c.rows >> (2 - l); m->lw[l] = c.cols >> (2 - l); }
}

// Conv2d weight [N][Cin][3][3] -> rows row(n) of dst [.][9 * Cpad], k = (ky * 3 + kx) * Cpad + c (channels Cin .. Cpad - 1 stay 0)
template <class T, class F>
void crnn_pack3(const T *w, int N, int Cin, int Cpad, F row, T *dst) {
  for (int n = 0; n < N; ++n)
    for (int c = 0; c < Cin; ++c)
      for (int t = 0; t < 9; ++t) dst[(size_t)row(n) * 9 * Cpad + (size_t)t * Cpad + c] = w[((size_t)n * Cin + c) * 9 + t];
}

// ConvTranspose2d weight [Cin][N][4][4] -> [4 parity classes (py, px)][N][4 * Cin], k = (ty * 2 + tx) * Cin + c: output
// (2 qy + py, 2 qx + px) reads input (qy + py - ty, qx + px - tx) through weight tap (1 - py + 2 ty, 1 - px + 2 tx)
template <class T>
std::vector<T> crnn_pack_t4(const T *w, int Cin, int N) {
  std::vector<T> out((size_t)16 * N * Cin);
  for (int cls = 0; cls < 4; ++cls)
    for (int n = 0; n < N; ++n)
      for (int tap = 0; tap < 4; ++tap)
        for (int c = 0; c < Cin; ++c) {
          const int ky = 1 - (cls >> 1) + 2 * (tap >> 1), kx = 1 - (cls & 1) + 2 * (tap & 1);
          out[(((size_t)cls * N + n) * 4 + tap) * Cin + c] = w[(((size_t)c * N + n) * 4 + ky) * 4 + kx];
        }
  return out;
}

// Packed weights of layer i: `w0` and, for a GRU cell, `w1` (the candidate conv).  GRU gates: rows [0, hid) reset_gate,
// [hid, 2 hid) update_gate.  LSTM: row 4 ch + gate of the packed matrix is row gate * hid + ch of conv.weight (i, f, o, g).
// T = float packs values (src(j): tensor p0 + j of the layer); T = unsigned packs 1-based indices into the flat master
// weights, 0 where the packed layout holds a padding zero (cm_convrnn_train_host.inc).
template <class T, class S>
void crnn_pack_layer_t(const cm_convrnn *m, int i, S src, std::vector<T> *w0, std::vector<T> *w1) {
  const CrnnLayer &l = m->L[i];
  w1->clear();
  if (l.kind == CRNN_UP) { *w0 = crnn_pack_t4<T>(src(0), l.cin, l.cout); return; }
  if (l.kind != CRNN_CELL) {
    const int cpad = (l.cin + 7) / 8 * 8;
    w0->assign((size_t)l.cout * 9 * cpad, T(0));
    crnn_pack3(src(0), l.cout, l.cin, cpad, [](int n) { return n; }, w0->data());
    return;
  }
  const int hid = l.cout, cin = l.cin + hid;
  if (m->cfg.cell == CM_CELL_GRU) {
    w0->assign((size_t)2 * hid * 9 * cin, T(0));
    crnn_pack3(src(0), hid, cin, cin, [](int n) { return n; }, w0->data());
    crnn_pack3(src(1), hid, cin, cin, [hid](int n) { return hid + n; }, w0->data());
    w1->assign((size_t)hid * 9 * cin, T(0));
    crnn_pack3(src(2), hid, cin, cin, [](int n) { return n; }, w1->data());
  } else {
    w0->assign((size_t)4 * hid * 9 * cin, T(0));
    crnn_pack3(src(0), 4 * hid, cin, cin, [hid](int n) { return 4 * (n % hid) + n / hid; }, w0->data());
  }
}

void crnn_pack_layer(const cm_convrnn *m, int i, std::vector<float> *w0, std::vector<float> *w1) {
  const Param *p = &m->params[m->L[i].p0];
  crnn_pack_layer_t<float>(m, i, [p](int j) { return p[j].host.data(); }, w0, w1);
}

int crnn_alloc(cm_convrnn *m, float **p, size_t n) {
  CM_HIP(hipMalloc((void **)p, std::max<size_t>(n, 8) * sizeof(float)));
  m->allocs.push_back(*p);
  return 0;
}

const Param *crnn_find(const cm_convrnn *m, const char *name) {
  for (const Param &p : m->params)
    if (p.name == name) return &p;
  return nullptr;
}

cm::CrnnConvArgs crnn_args(const cm_convrnn *m, int geo, int epi, const float *W, int B, int lin, int lout,
                           const _Float16 *Wh = nullptr) {
  cm::CrnnConvArgs a{};
  a.geo = geo; a.epi = epi; a.W = W; a.Wh = Wh; a.B = B;
  a.Hi = m->lh[lin]; a.Wi = m->lw[lin]; a.Ho = m->lh[lout]; a.Wo = m->lw[lout];
  return a;
}

// One recurrent cell on hidden state `level`: x [B][h][w][Cx] is its input (Cx = the layer's input_dim)
int crnn_cell(cm_convrnn *m, const CrnnLayer &l, const float *x, int B, hipStream_t st) {
  const int lv = l.level, hid = l.cout;
  const long long pix = (long long)m->lh[lv] * m->lw[lv];
  float *hp = m->h[lv][m->cur[lv]], *hn = m->h[lv][m->cur[lv] ^ 1];
  cm::CrnnConvArgs a = crnn_args(m, cm::CRNN_GEO_S1, 0, l.w0, B, lv, lv, l.h0);
  a.x0 = x; a.bs0 = pix * l.cin; a.C0 = l.cin;
  a.x1 = hp; a.bs1 = pix * hid; a.C1 = hid;
  if (m->cfg.cell == CM_CELL_GRU) {
    a.epi = cm::CRNN_EPI_GRU_GATES; a.N = 2 * hid; a.y = m->scr; a.u = m->u; a.hprev = hp;
    CM_HIP(cm::launch_crnn_conv(a, st));
    a.epi = cm::CRNN_EPI_GRU_CAND; a.N = hid; a.W = l.w1; a.Wh = l.h1; a.x1 = m->scr; a.y = hn;
    CM_HIP(cm::launch_crnn_conv(a, st));
  } else {
    a.epi = cm::CRNN_EPI_LSTM; a.N = 4 * hid; a.y = hn; a.c = m->c[lv];
    CM_HIP(cm::launch_crnn_conv(a, st));
  }
  m->cur[lv] ^= 1;
  return 0;
}

// A plain conv layer with LeakyReLU: x at level `lin` -> y at level l.level
int crnn_conv(cm_convrnn *m, const CrnnLayer &l, const float *x, long long bs, int cx, int lin, float *y, int B, hipStream_t st) {
  const int geo = l.kind == CRNN_UP ? cm::CRNN_GEO_T4 : l.kind == CRNN_DOWN ? cm::CRNN_GEO_S2 : cm::CRNN_GEO_S1;
  cm::CrnnConvArgs a = crnn_args(m, geo, cm::CRNN_EPI_LEAKY, l.w0, B, lin, l.level, l.h0);
  a.x0 = x; a.bs0 = bs; a.C0 = cx; a.N = l.cout; a.y = y;
  CM_HIP(cm::launch_crnn_conv(a, st));
  return 0;
}

int crnn_run(cm_convrnn *m, const float *d_past, const float *d_target, int tf, int exp_output, float *d_out, int B, hipStream_t st) {
  const cm_convrnn_config &c = m->cfg;
  const int H = c.rows, W = c.cols, P = c.past_len, Ft = c.future_len, nslots = P + Ft;
  const long long HW = (long long)H * W, win_bs = (long long)nslots * HW * 8;
  m->tape_ready = false;          // the window is rewritten
  for (int l = 0; l < 3; ++l) {   // _init_hidden: zero states at the start of every call (forecaster.py:99)
    const size_t n = (size_t)B * m->lh[l] * m->lw[l] * m->hid[l] * sizeof(float);
    CM_HIP(hipMemsetAsync(m->h[l][0], 0, n, st));
    if (m->c[l]) CM_HIP(hipMemsetAsync(m->c[l], 0, n, st));
    m->cur[l] = 0;
  }
  CM_HIP(cm::launch_crnn_pack_frames(d_past, m->win, B, H, W, P, nslots, 0, st));
  if (tf) CM_HIP(cm::launch_crnn_pack_frames(d_target, m->win, B, H, W, Ft, nslots, P, st));
  CrnnLayer *L = m->L;
  for (int t = 0; t < Ft; ++t) {
    for (int p = 0; p < P; ++p) {   // encoder.py:91-135
      if (crnn_conv(m, L[0], m->win + (long long)(t + p) * HW * 8, win_bs, 8, 2, m->act[0], B, st)) return 1;
      if (crnn_cell(m, L[1], m->act[0], B, st)) return 1;
      if (crnn_conv(m, L[2], m->h[2][m->cur[2]], HW * m->hid[2], m->hid[2], 2, m->act[1], B, st)) return 1;
      if (crnn_cell(m, L[3], m->act[1], B, st)) return 1;
      if (crnn_conv(m, L[4], m->h[1][m->cur[1]], HW / 4 * m->hid[1], m->hid[1], 1, m->act[2], B, st)) return 1;
      if (crnn_cell(m, L[5], m->act[2], B, st)) return 1;
    }
    // forecaster.py:112-159: frnn1's input is the encoder's last h, which is hs[0] itself
    if (crnn_cell(m, L[6], m->h[0][m->cur[0]], B, st)) return 1;
    if (crnn_conv(m, L[7], m->h[0][m->cur[0]], HW / 16 * m->hid[0], m->hid[0], 0, m->act[3], B, st)) return 1;
    if (crnn_cell(m, L[8], m->act[3], B, st)) return 1;
    if (crnn_conv(m, L[9], m->h[1][m->cur[1]], HW / 4 * m->hid[1], m->hid[1], 1, m->act[4], B, st)) return 1;
    if (crnn_cell(m, L[10], m->act[4], B, st)) return 1;
    if (crnn_conv(m, L[11], m->h[2][m->cur[2]], HW * m->hid[2], m->hid[2], 2, m->act[5], B, st)) return 1;
    cm::CrnnConvArgs a = crnn_args(m, cm::CRNN_GEO_S1, cm::CRNN_EPI_LAST, L[12].w0, B, 2, 2);
    a.x0 = m->act[5]; a.bs0 = HW * L[12].cin; a.C0 = L[12].cin; a.N = c.in_channels;
    a.out = d_out; a.Ft = Ft; a.t = t; a.exp_out = exp_output;
    a.win = tf ? nullptr : m->win + (long long)(P + t) * HW * 8; a.win_bs = win_bs;
    CM_HIP(cm::launch_crnn_conv(a, st));
  }
  m->lastB = B;
  return 0;
}

int crnn_ready(const cm_convrnn *m, int B) {
  if (!m) return fail("null ConvRNN handle");
  if (!m->finalized) return fail("cm_convrnn_finalize has not been called");
  if (B < 1 || B > m->cfg.max_batch) return fail("batch %d outside [1, max_batch=%d]", B, m->cfg.max_batch);
  return 0;
}

}  // namespace

extern "C" {

int cm_convrnn_create(const cm_convrnn_config *cfg, cm_convrnn **out) {
  if (!cfg || !out) return fail("null argument");
  static const int32_t EK[6] = {3, 3, 3, 3, 3, 3}, FK[7] = {3, 4, 3, 4, 3, 3, 3};
  const int32_t *E = cfg->enc_hidden, *F = cfg->forc_hidden;
  if (cfg->in_channels != 4) return fail("ConvRNN: in_channels must be 4 (the forecaster indexes channels 0 and 3), got %d", cfg->in_channels);
  if (cfg->rows < 4 || cfg->cols < 4 || cfg->rows % 4 || cfg->cols % 4)
    return fail("ConvRNN: rows and cols must be positive multiples of 4 (two stride-2 levels), got %d x %d", cfg->rows, cfg->cols);
  if (cfg->past_len < 1) return fail("ConvRNN: past_len must be >= 1, got %d", cfg->past_len);
  if (cfg->future_len < 1) return fail("ConvRNN: future_len must be >= 1, got %d", cfg->future_len);
  if (cfg->cell != CM_CELL_GRU && cfg->cell != CM_CELL_LSTM) return fail("ConvRNN: cell must be CM_CELL_GRU or CM_CELL_LSTM, got %d", cfg->cell);
  if (memcmp(cfg->enc_kernels, EK, sizeof(EK))) return fail("ConvRNN: enc_kernels must be [3,3,3,3,3,3] (padding is hard-wired to 1)");
  if (memcmp(cfg->forc_kernels, FK, sizeof(FK))) return fail("ConvRNN: forc_kernels must be [3,4,3,4,3,3,3] (padding is hard-wired to 1)");
  for (int i = 0; i < 13; ++i) {
    const int v = i < 6 ? E[i] : F[i - 6];
    if (v < 8 || v % 8 || v > 1024)
      return fail("ConvRNN: %s[%d] = %d: channel counts must be multiples of 8 in [8, 1024]", i < 6 ? "enc_hidden" : "forc_hidden", i < 6 ? i : i - 6, v);
  }
  if (E[2] != E[1]) return fail("ConvRNN: feed-through enc_hidden[2] == enc_hidden[1] violated (%d vs %d): ernn2 is built for enc_hidden[1] input channels", E[2], E[1]);
  if (E[4] != E[3]) return fail("ConvRNN: feed-through enc_hidden[4] == enc_hidden[3] violated (%d vs %d): ernn3 is built for enc_hidden[3] input channels", E[4], E[3]);
  if (F[0] != E[5]) return fail("ConvRNN: feed-through forc_hidden[0] == enc_hidden[5] violated (%d vs %d): frnn1 is fed the encoder's last h", F[0], E[5]);
  if (F[1] != E[5]) return fail("ConvRNN: shared state forc_hidden[1] == enc_hidden[5] violated (%d vs %d): both cells run on hs[0]", F[1], E[5]);
  if (F[3] != E[3]) return fail("ConvRNN: shared state forc_hidden[3] == enc_hidden[3] violated (%d vs %d): both cells run on hs[1]", F[3], E[3]);
  if (F[5] != E[1]) return fail("ConvRNN: shared state forc_hidden[5] == enc_hidden[1] violated (%d vs %d): both cells run on hs[2]", F[5], E[1]);
  if (cfg->max_batch < 1) return fail("ConvRNN: max_batch must be >= 1");
  if ((long long)cfg->max_batch * cfg->rows * cfg->cols > 0x7fffffffLL - 64)
    return fail("ConvRNN: max_batch * rows * cols = %lld exceeds the 2^31 - 64 pixel rows one launch indexes",
                (long long)cfg->max_batch * cfg->rows * cfg->cols);
  if (cfg->device >= 0) {
    int ndev = 0;
    CM_HIP(hipGetDeviceCount(&ndev));
    if (cfg->device >= ndev) return fail("device %d not available (%d devices)", cfg->device, ndev);
  }
  auto m = std::make_unique<cm_convrnn>();
  m->cfg = *cfg;
  m->device = cfg->device;
  crnn_build(m.get());
  if (m->device >= 0) {
    DevGuard g(m->device);
    CM_HIP(hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking));
  }
  *out = m.release();
  return 0;
}

int cm_convrnn_destroy(cm_convrnn *m) {
  if (!m) return 0;
  if (m->device >= 0) {
    DevGuard g(m->device);
    hipDeviceSynchronize();
    for (void *p : m->allocs) hipFree(p);
    if (m->stream) hipStreamDestroy(m->stream);
  }
  crnn_free_train(m->train);
  delete m;
  return 0;
}

int cm_convrnn_num_params(const cm_convrnn *m, int32_t *count) {
  if (!m || !count) return fail("null argument");
  *count = (int32_t)m->params.size();
  return 0;
}

int cm_convrnn_param_info(const cm_convrnn *m, int32_t index, const char **name, int64_t shape[4], int32_t *ndim) {
  if (!m || !name || !shape || !ndim) return fail("null argument");
  if (index < 0 || index >= (int32_t)m->params.size()) return fail("parameter index %d out of range", index);
  const Param &p = m->params[index];
  *name = p.name.c_str();
  *ndim = (int32_t)p.shape.size();
  for (int i = 0; i < 4; ++i) shape[i] = i < *ndim ? p.shape[i] : 0;
  return 0;
}

int cm_convrnn_set_param(cm_convrnn *m, const char *name, const float *h_data, int64_t numel) {
  if (!m || !name || !h_data) return fail("null argument");
  Param *p = const_cast<Param *>(crnn_find(m, name));
  if (!p) return fail("unknown ConvRNN parameter '%s'", name);
  if (numel != p->numel()) return fail("parameter '%s' has %lld elements, got %lld", name, (long long)p->numel(), (long long)numel);
  if (m->finalized) return fail("cm_convrnn_set_param after cm_convrnn_finalize: create a new handle");
  memcpy(p->host.data(), h_data, (size_t)numel * sizeof(float));
  p->set = true;
  return 0;
}

int cm_convrnn_get_param(const cm_convrnn *m, const char *name, float *h_data, int64_t numel) {
  if (!m || !name || !h_data) return fail("null argument");
  const Param *p = crnn_find(m, name);
  if (!p) return fail("unknown ConvRNN parameter '%s'", name);
  if (numel != p->numel()) return fail("parameter '%s' has %lld elements, got %lld", name, (long long)p->numel(), (long long)numel);
  memcpy(h_data, p->host.data(), (size_t)numel * sizeof(float));
  return 0;
}

int cm_convrnn_set_precision(cm_convrnn *m, int32_t precision) {
  if (!m) return fail("null ConvRNN handle");
  if (precision == CM_PRECISION_F32R || precision == CM_PRECISION_F32X)
    return fail("ConvRNN: CM_PRECISION_F32R / CM_PRECISION_F32X are conv split forms of the UNet; a ConvRNN handle takes "
                "CM_PRECISION_F32 or CM_PRECISION_F16");
  if (precision != CM_PRECISION_F32 && precision != CM_PRECISION_F16) return fail("unknown precision %d", precision);
  if (m->finalized) return fail("cm_convrnn_set_precision after cm_convrnn_finalize: create a new handle");
  m->precision = precision;
  return 0;
}

int cm_convrnn_finalize(cm_convrnn *m) {
  if (!m) return fail("null ConvRNN handle");
  if (m->device < 0) return fail("host-only ConvRNN handle (device < 0) cannot be finalized");
  if (m->finalized) return 0;
  for (const Param &p : m->params)
    if (!p.set) return fail("parameter '%s' was never set", p.name.c_str());
  DevGuard g(m->device);
  const cm_convrnn_config &c = m->cfg;
  std::vector<float> w0, w1;
  std::vector<_Float16> h16;
  for (int i = 0; i < 13; ++i) {
    crnn_pack_layer(m, i, &w0, &w1);
    if (m->precision == CM_PRECISION_F16 && i >= 1 && i <= 11) {   // the f16 plan's operands; layers 0 and 12 stay fp32
      for (int j = 0; j < 2; ++j) {
        const std::vector<float> &w = j ? w1 : w0;
        if (w.empty()) continue;
        h16.resize(w.size());
        for (size_t e = 0; e < w.size(); ++e) h16[e] = (_Float16)w[e];   // round-to-nearest-even, no clamp (as dit_finalize)
        _Float16 *dp = nullptr;
        CM_HIP(hipMalloc((void **)&dp, std::max<size_t>(h16.size(), 8) * sizeof(_Float16)));
        m->allocs.push_back(dp);
        CM_HIP(hipMemcpy(dp, h16.data(), h16.size() * sizeof(_Float16), hipMemcpyHostToDevice));
        (j ? m->L[i].h1 : m->L[i].h0) = dp;
      }
      continue;
    }
    if (crnn_alloc(m, &m->L[i].w0, w0.size())) return 1;
    CM_HIP(hipMemcpy(m->L[i].w0, w0.data(), w0.size() * sizeof(float), hipMemcpyHostToDevice));
    if (w1.empty()) continue;
    if (crnn_alloc(m, &m->L[i].w1, w1.size())) return 1;
    CM_HIP(hipMemcpy(m->L[i].w1, w1.data(), w1.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  const size_t MB = (size_t)c.max_batch, HW = (size_t)c.rows * c.cols;
  if (crnn_alloc(m, &m->win, MB * (c.past_len + c.future_len) * HW * 8)) return 1;
  CM_HIP(hipMemset(m->win, 0, MB * (c.past_len + c.future_len) * HW * 8 * sizeof(float)));
  const size_t act_n[6] = {HW * c.enc_hidden[0], HW / 4 * c.enc_hidden[2], HW / 16 * c.enc_hidden[4],
                           HW / 4 * c.forc_hidden[2], HW * c.forc_hidden[4], HW * c.forc_hidden[6]};
  for (int i = 0; i < 6; ++i)
    if (crnn_alloc(m, &m->act[i], MB * act_n[i])) return 1;
  size_t smax = 0;
  for (int l = 0; l < 3; ++l) {
    const size_t n = MB * m->lh[l] * m->lw[l] * m->hid[l];
    smax = std::max(smax, n);
    if (crnn_alloc(m, &m->h[l][0], n) || crnn_alloc(m, &m->h[l][1], n)) return 1;
    if (c.cell == CM_CELL_LSTM && crnn_alloc(m, &m->c[l], n)) return 1;
  }
  if (crnn_alloc(m, &m->scr, smax)) return 1;   // r * h_prev of a GRU cell; the transposed copy of cm_convrnn_debug_state
  if (c.cell == CM_CELL_GRU && crnn_alloc(m, &m->u, smax)) return 1;
  if (crnn_alloc(m, &m->st_past, MB * 4 * HW * c.past_len) || crnn_alloc(m, &m->st_tgt, MB * 4 * HW * c.future_len) ||
      crnn_alloc(m, &m->st_out, MB * 4 * HW * c.future_len))
    return 1;
  m->finalized = true;
  return 0;
}

int cm_convrnn_forecast(cm_convrnn *m, const float *d_past, const float *d_target, int32_t teacher_forcing, int32_t exp_output,
                        float *d_out, int32_t B, void *stream) {
  if (crnn_ready(m, B)) return 1;
  if (!d_past || !d_out) return fail("null argument");
  if (teacher_forcing && !d_target) return fail("teacher_forcing needs d_target");
  DevGuard g(m->device);
  return crnn_run(m, d_past, d_target, teacher_forcing != 0, exp_output != 0, d_out, B, stream ? (hipStream_t)stream : m->stream);
}

int cm_convrnn_forecast_host(cm_convrnn *m, const float *h_past, const float *h_target, int32_t teacher_forcing, int32_t exp_output,
                             float *h_out, int32_t B) {
  if (crnn_ready(m, B)) return 1;
  if (!h_past || !h_out) return fail("null argument");
  if (teacher_forcing && !h_target) return fail("teacher_forcing needs h_target");
  DevGuard g(m->device);
  const cm_convrnn_config &c = m->cfg;
  const size_t per = (size_t)B * 4 * c.rows * c.cols * sizeof(float);
  CM_HIP(hipMemcpyAsync(m->st_past, h_past, per * c.past_len, hipMemcpyHostToDevice, m->stream));
  if (teacher_forcing) CM_HIP(hipMemcpyAsync(m->st_tgt, h_target, per * c.future_len, hipMemcpyHostToDevice, m->stream));
  if (crnn_run(m, m->st_past, m->st_tgt, teacher_forcing != 0, exp_output != 0, m->st_out, B, m->stream)) return 1;
  CM_HIP(hipMemcpyAsync(h_out, m->st_out, per * c.future_len, hipMemcpyDeviceToHost, m->stream));
  CM_HIP(hipStreamSynchronize(m->stream));
  return 0;
}

int cm_convrnn_debug_state(cm_convrnn *m, int32_t level, int32_t which, float *h_out, int64_t capacity, int64_t shape[4]) {
  if (!m || !h_out || !shape) return fail("null argument");
  if (!m->finalized || m->lastB < 1) return fail("no forecast has run on this handle");
  if (level < 0 || level > 2) return fail("level %d outside [0, 2]", level);
  if (which != 0 && !(which == 1 && m->cfg.cell == CM_CELL_LSTM)) return fail("state %d: a GRU handle has only h (0); an LSTM handle h (0) and c (1)", which);
  const int B = m->lastB, C = m->hid[level], h = m->lh[level], w = m->lw[level];
  const int64_t n = (int64_t)B * C * h * w;
  if (capacity < n) return fail("capacity %lld < %lld elements", (long long)capacity, (long long)n);
  DevGuard g(m->device);
  const float *src = which ? m->c[level] : m->h[level][m->cur[level]];
  CM_HIP(hipStreamSynchronize(m->stream));
  CM_HIP(cm::launch_crnn_state_nchw(src, m->scr, B, C, h, w, m->stream));
  CM_HIP(hipMemcpyAsync(h_out, m->scr, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, m->stream));
  CM_HIP(hipStreamSynchronize(m->stream));
  shape[0] = B; shape[1] = C; shape[2] = h; shape[3] = w;
  return 0;
}

namespace {

// host [B][C][h][w] -> a fresh device buffer [B][h][w][Cpad] (channels C .. Cpad - 1 zero); null stays null
int crnn_dbg_up(const float *src, int B, int C, int Cpad, int h, int w, std::vector<void *> *owned, float **dst) {
  *dst = nullptr;
  if (!src) return 0;
  std::vector<float> t((size_t)B * h * w * Cpad, 0.f);
  for (int b = 0; b < B; ++b)
    for (int c = 0; c < C; ++c)
      for (int p = 0; p < h * w; ++p) t[((size_t)b * h * w + p) * Cpad + c] = src[((size_t)b * C + c) * h * w + p];
  CM_HIP(hipMalloc((void **)dst, t.size() * sizeof(float)));
  owned->push_back(*dst);
  CM_HIP(hipMemcpy(*dst, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice));
  return 0;
}

// a device buffer [B][h][w][C] -> host [B][C][h][w]
int crnn_dbg_down(const float *src, int B, int C, int h, int w, float *dst) {
  std::vector<float> t((size_t)B * h * w * C);
  CM_HIP(hipMemcpy(t.data(), src, t.size() * sizeof(float), hipMemcpyDeviceToHost));
  for (int b = 0; b < B; ++b)
    for (int c = 0; c < C; ++c)
      for (int p = 0; p < h * w; ++p) dst[((size_t)b * C + c) * h * w + p] = t[((size_t)b * h * w + p) * C + c];
  return 0;
}

int crnn_debug_launch(cm_convrnn *m, int i, int part, const float *h_x0, const float *h_x1, const float *h_hprev, const float *h_u,
                      const float *h_c, float *h_y0, float *h_y1, int B, std::vector<void *> *owned) {
  const CrnnLayer &l = m->L[i];
  const bool gru = m->cfg.cell == CM_CELL_GRU;
  const int lout = l.level, lin = l.kind == CRNN_DOWN ? lout + 1 : l.kind == CRNN_UP ? lout - 1 : lout;
  const int hi = m->lh[lin], wi = m->lw[lin], ho = m->lh[lout], wo = m->lw[lout];
  const int cpad = (l.cin + 7) / 8 * 8;
  float *x0 = nullptr, *x1 = nullptr, *hp = nullptr, *u = nullptr, *c = nullptr, *y0 = nullptr, *y1 = nullptr;
  auto fresh = [&](float **p, size_t n) {
    CM_HIP(hipMalloc((void **)p, n * sizeof(float)));
    owned->push_back(*p);
    CM_HIP(hipMemset(*p, 0, n * sizeof(float)));
    return 0;
  };
  if (crnn_dbg_up(h_x0, B, l.cin, cpad, hi, wi, owned, &x0)) return 1;
  if (l.kind != CRNN_CELL) {
    if (part != 0) return fail("layer %d is a conv: it has part 0 only", i);
    const int geo = l.kind == CRNN_UP ? cm::CRNN_GEO_T4 : l.kind == CRNN_DOWN ? cm::CRNN_GEO_S2 : cm::CRNN_GEO_S1;
    if (fresh(&y0, (size_t)B * ho * wo * l.cout)) return 1;
    cm::CrnnConvArgs a = crnn_args(m, geo, cm::CRNN_EPI_LEAKY, l.w0, B, lin, lout, l.h0);
    a.x0 = x0; a.bs0 = (long long)hi * wi * cpad; a.C0 = cpad; a.N = l.cout; a.y = y0;
    CM_HIP(cm::launch_crnn_conv(a, m->stream));
    CM_HIP(hipStreamSynchronize(m->stream));
    return crnn_dbg_down(y0, B, l.cout, ho, wo, h_y0);
  }
  const int hid = l.cout;
  const size_t ns = (size_t)B * ho * wo * hid;
  if (part != 0 && !(part == 1 && gru)) return fail("layer %d: part %d (0: the GRU gates or the LSTM; 1: the GRU candidate)", i, part);
  if (!h_x1) return fail("a cell launch needs x1");
  if (gru ? !h_hprev || (part == 1 && !h_u) : !h_c) return fail("a cell launch needs hprev (GRU; its candidate u as well) or c (LSTM)");
  if (!gru || part == 0) { if (!h_y1) return fail("this launch has two outputs: y1 is null"); }
  if (crnn_dbg_up(h_x1, B, hid, hid, ho, wo, owned, &x1) || crnn_dbg_up(h_hprev, B, hid, hid, ho, wo, owned, &hp) ||
      crnn_dbg_up(h_u, B, hid, hid, ho, wo, owned, &u) || crnn_dbg_up(h_c, B, hid, hid, ho, wo, owned, &c))
    return 1;
  if (fresh(&y0, ns) || fresh(&y1, ns)) return 1;
  const long long pix = (long long)ho * wo;
  cm::CrnnConvArgs a = crnn_args(m, cm::CRNN_GEO_S1, 0, l.w0, B, lout, lout, l.h0);
  a.x0 = x0; a.bs0 = pix * l.cin; a.C0 = l.cin;
  a.x1 = x1; a.bs1 = pix * hid; a.C1 = hid;
  if (gru && part == 0) {
    a.epi = cm::CRNN_EPI_GRU_GATES; a.N = 2 * hid; a.y = y0; a.u = y1; a.hprev = hp;
  } else if (gru) {
    a.epi = cm::CRNN_EPI_GRU_CAND; a.N = hid; a.W = l.w1; a.Wh = l.h1; a.y = y0; a.u = u; a.hprev = hp;
  } else {
    a.epi = cm::CRNN_EPI_LSTM; a.N = 4 * hid; a.y = y0; a.c = c; a.cn = y1;
  }
  CM_HIP(cm::launch_crnn_conv(a, m->stream));
  CM_HIP(hipStreamSynchronize(m->stream));
  if (crnn_dbg_down(y0, B, hid, ho, wo, h_y0)) return 1;
  if (!gru || part == 0) return crnn_dbg_down(y1, B, hid, ho, wo, h_y1);
  return 0;
}

}  // namespace

int cm_convrnn_debug_launch(cm_convrnn *m, int32_t layer, int32_t part, const float *h_x0, const float *h_x1, const float *h_hprev,
                            const float *h_u, const float *h_c, float *h_y0, float *h_y1, int32_t B) {
  if (crnn_ready(m, B)) return 1;
  if (layer < 0 || layer > 11) return fail("layer %d outside [0, 11] (the last conv writes the forecast itself: cm_convrnn_forecast)", layer);
  if (!h_x0 || !h_y0) return fail("null argument");
  DevGuard g(m->device);
  std::vector<void *> owned;
  const int rc = crnn_debug_launch(m, layer, part, h_x0, h_x1, h_hprev, h_u, h_c, h_y0, h_y1, B, &owned);
  hipDeviceSynchronize();
  for (void *p : owned) hipFree(p);
  return rc;
}

// Algorithmic FLOPs (2 per multiply-add of the reference's convolutions; a transposed 4x4 stride-2 conv has 4 taps per
// output) and the bytes of every launch's sources, output and weights, of one forecast at batch B.  On the f16 plan the
// weights of layers 1-11 are two bytes each; every tensor a launch reads or writes is fp32 on either plan.
int cm_convrnn_cost(const cm_convrnn *m, int32_t B, double *flops, double *bytes) {
  if (!m || !flops || !bytes) return fail("null argument");
  if (B < 1) return fail("batch must be >= 1");
  double f[2] = {0, 0}, by[2] = {0, 0};   // encoder (per frame), forecaster (per step)
  for (int i = 0; i < 13; ++i) {
    const CrnnLayer &l = m->L[i];
    const double wb = m->precision == CM_PRECISION_F16 && i >= 1 && i <= 11 ? 2 : 4;   // bytes of a weight; tensors stay fp32
    const double pout = (double)B * m->lh[l.level] * m->lw[l.level];
    const double pin = l.kind == CRNN_DOWN ? pout * 4 : l.kind == CRNN_UP ? pout / 4 : pout;
    double macs, bts;
    if (l.kind == CRNN_CELL) {
      const double cin = l.cin + l.cout, ngate = m->cfg.cell == CM_CELL_GRU ? 3 : 4;
      macs = pout * ngate * l.cout * 9 * cin;
      bts = 4 * ((m->cfg.cell == CM_CELL_GRU ? 2 : 1) * pout * cin + pout * l.cout * (m->cfg.cell == CM_CELL_GRU ? 5 : 4)) +
            wb * ngate * l.cout * 9 * cin;
    } else {
      const double taps = l.kind == CRNN_UP ? 4 : 9;
      macs = pout * l.cout * taps * l.cin;
      bts = 4 * (pin * l.cin + pout * l.cout) + wb * (l.kind == CRNN_UP ? 16.0 : 9.0) * l.cout * l.cin;
    }
    f[i >= 6] += 2 * macs;
    by[i >= 6] += bts;
  }
  *flops = m->cfg.future_len * (m->cfg.past_len * f[0] + f[1]);
  *bytes = m->cfg.future_len * (m->cfg.past_len * by[0] + by[1]);
  return 0;
}

}  // extern "C"

#include "cm_convrnn_train_host.inc"
