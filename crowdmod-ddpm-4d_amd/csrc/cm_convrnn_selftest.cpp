// Host-side self-test of the ConvRNN handle (cm_convrnn_host.inc), built by `make asan` next to cm_host_selftest and run
// under ASan / UBSan as a stand-alone program: no kernel is launched, no device is needed.  Host-only handles (device < 0)
// of both cell classes: creation, one refusal per constraint, state_dict enumeration, set / get round trips and their
// refusals, and the weight packers checked element by element against their definitions.
#include "cm_model.cpp"

#include <cstdio>

namespace {

int failures = 0;
#define EXPECT(cond)                                                                  \
  do {                                                                                \
    if (!(cond)) { fprintf(stderr, "%s:%d: EXPECT(%s) failed\n", __FILE__, __LINE__, #cond); ++failures; } \
  } while (0)

cm_convrnn_config base_cfg(int cell) {
  cm_convrnn_config c{};
  c.in_channels = 4; c.rows = 12; c.cols = 20; c.past_len = 5; c.future_len = 3; c.cell = cell;
  const int E[6] = {16, 40, 40, 72, 72, 72}, F[7] = {72, 72, 72, 72, 72, 40, 24}, EK[6] = {3, 3, 3, 3, 3, 3}, FK[7] = {3, 4, 3, 4, 3, 3, 3};
  for (int i = 0; i < 6; ++i) { c.enc_hidden[i] = E[i]; c.enc_kernels[i] = EK[i]; }
  for (int i = 0; i < 7; ++i) { c.forc_hidden[i] = F[i]; c.forc_kernels[i] = FK[i]; }
  c.max_batch = 2; c.device = -1;
  return c;
}

template <class F>
void refused(F &&edit, const char *what) {
  cm_convrnn_config c = base_cfg(CM_CELL_GRU);
  edit(c);
  cm_convrnn *h = nullptr;
  const int rc = cm_convrnn_create(&c, &h);
  if (rc == 0 || !strstr(cm_last_error(), what)) {
    fprintf(stderr, "refusal '%s': rc %d, message '%s'\n", what, rc, rc ? cm_last_error() : "");
    ++failures;
  }
  if (rc == 0) cm_convrnn_destroy(h);
}

float wval(int tensor, size_t i) { return (float)((tensor * 7919 + (int)(i % 100003)) % 2003) - 1001.f; }

// The backward weight layouts (cm_convrnn_train_host.inc) against a direct index computation on the state_dict tensors, as
// values and as the 1-based index tables the device re-packs and reduces through.
void test_train_packs(const cm_convrnn *m, int cell) {
  const OptLayout lay = opt_layout(m->params, {});   // as cm_convrnn_train_init lays the store out
  const std::vector<size_t> &off = lay.off;
  const size_t total = lay.nfloats;
  std::vector<unsigned> ids(total);
  for (size_t k = 0; k < total; ++k) ids[k] = (unsigned)(k + 1);
  const bool gru = cell == CM_CELL_GRU;
  std::vector<float> fv[2], bv[2];
  std::vector<unsigned> fi[2], bi[2];
  for (int i = 0; i < 13; ++i) {
    const CrnnLayer &l = m->L[i];
    const Param *pp = &m->params[l.p0];
    const size_t *po = &off[l.p0];
    crnn_pack_train_t<float>(m, i, [&](int j) { return pp[j].host.data(); }, fv, bv);
    crnn_pack_train_t<unsigned>(m, i, [&](int j) { return ids.data() + po[j]; }, fi, bi);
    // weight of conv j: output channel n (in the packed row order), input channel c, tap (ky, kx): tensor and flat element
    auto elem = [&](int j, int n, int c, int ky, int kx, int *tensor, size_t *e) {
      if (l.kind == CRNN_UP) { *tensor = 0; *e = (((size_t)c * l.cout + n) * 4 + ky) * 4 + kx; return; }
      const int cin = l.kind == CRNN_CELL ? l.cin + l.cout : l.cin;
      int t = 0, row = n;
      if (l.kind == CRNN_CELL && gru) { t = j ? 2 : n / l.cout; row = j ? n : n % l.cout; }
      if (l.kind == CRNN_CELL && !gru) row = (n % 4) * l.cout + n / 4;
      *tensor = t; *e = (((size_t)row * cin + c) * 3 + ky) * 3 + kx;
    };
    size_t seen = 0;
    for (int j = 0; j < 2; ++j) {
      if (bv[j].empty()) continue;
      EXPECT(bv[j].size() == bi[j].size() && fv[j].size() == fi[j].size());
      const bool cellk = l.kind == CRNN_CELL;
      const int N = cellk ? (j ? 1 : gru ? 2 : 4) * l.cout : l.cout, Nr = (N + 7) / 8 * 8;
      const int cin = cellk ? l.cin + l.cout : l.cin, cpad = (cin + 7) / 8 * 8;
      std::vector<char> hit(bv[j].size(), 0);
      auto check = [&](size_t at, int n, int c, int ky, int kx) {
        int t; size_t e;
        elem(j, n, c, ky, kx, &t, &e);
        if (at >= bv[j].size() || hit[at] || bv[j][at] != pp[t].host[e] || bi[j][at] != (unsigned)(po[t] + e + 1)) {
          fprintf(stderr, "backward pack differs in layer %d conv %d (n %d c %d tap %d %d)\n", i, j, n, c, ky, kx); ++failures; return false;
        }
        hit[at] = 1; ++seen;
        return true;
      };
      bool ok = true;
      if (l.kind == CRNN_UP) {          // [c][(ky * 4 + kx) * N + n]: dy(2 iy - 1 + ky, 2 ix - 1 + kx) meets x(iy, ix) through w[c][n][ky][kx]
        EXPECT(bv[j].size() == (size_t)cin * 16 * N);
        for (int c = 0; c < cin && ok; ++c)
          for (int ky = 0; ky < 4; ++ky)
            for (int kx = 0; kx < 4; ++kx)
              for (int n = 0; n < N && ok; ++n) ok = check(((size_t)c * 16 + ky * 4 + kx) * N + n, n, c, ky, kx);
      } else if (l.kind == CRNN_DOWN) { // input (2 qy + py, ...) = 2 oy + ky - 1 with oy = qy + py - ty: ky = 1 - py + 2 ty
        EXPECT(bv[j].size() == (size_t)9 * cin * N);
        size_t base = 0;
        for (int cls = 0; cls < 4; ++cls) {
          const int py = cls >> 1, px = cls & 1, nt = (1 + py) * (1 + px);
          for (int c = 0; c < cin && ok; ++c)
            for (int ty = 0; ty <= py; ++ty)
              for (int tx = 0; tx <= px; ++tx)
                for (int n = 0; n < N && ok; ++n) {
                  const int ky = 1 - py + 2 * ty, kx = 1 - px + 2 * tx;
                  EXPECT(2 * (py - ty) + ky - 1 == py && 2 * (px - tx) + kx - 1 == px);   // the tap does reach this parity
                  ok = check(base + ((size_t)c * nt + ty * (1 + px) + tx) * N + n, n, c, ky, kx);
                }
          base += (size_t)nt * cin * N;
        }
      } else {                          // [c][(ty * 3 + tx) * Nr + n]: dy(q + t - 1) met x(q) through tap (2 - ty, 2 - tx)
        EXPECT(bv[j].size() == (size_t)cpad * 9 * Nr);
        for (int c = 0; c < cin && ok; ++c)
          for (int ty = 0; ty < 3; ++ty)
            for (int tx = 0; tx < 3; ++tx)
              for (int n = 0; n < N && ok; ++n) ok = check(((size_t)c * 9 + ty * 3 + tx) * Nr + n, n, c, 2 - ty, 2 - tx);
      }
      if (!ok) return;
      for (size_t k = 0; k < hit.size(); ++k)
        if (!hit[k] && (bv[j][k] != 0.f || bi[j][k] != 0)) { fprintf(stderr, "padding of backward pack %d/%d is not zero\n", i, j); ++failures; return; }
      // the forward index table names the element the forward value came from
      for (size_t k = 0; k < fv[j].size(); ++k) {
        const unsigned id = fi[j][k];
        bool same = id ? false : fv[j][k] == 0.f;
        for (int t = 0; id && t < 3 && l.p0 + t < (int)m->params.size(); ++t)
          if (id > po[t] && id <= po[t] + pp[t].host.size()) same = pp[t].host[id - 1 - po[t]] == fv[j][k];
        if (!same) { fprintf(stderr, "forward index table differs in layer %d conv %d\n", i, j); ++failures; return; }
      }
    }
    size_t numel = 0;
    for (int t = 0; t < (l.kind == CRNN_CELL && gru ? 3 : 1); ++t) numel += pp[t].host.size();
    EXPECT(seen == numel);   // every weight exactly once
  }
}

void test_handle(int cell) {
  cm_convrnn_config c = base_cfg(cell);
  cm_convrnn *m = nullptr;
  EXPECT(cm_convrnn_create(&c, &m) == 0);
  if (!m) return;
  int32_t n = 0;
  EXPECT(cm_convrnn_num_params(m, &n) == 0 && n == (cell == CM_CELL_GRU ? 25 : 13));
  for (int i = 0; i < n; ++i) {
    const char *name = nullptr;
    int64_t shape[4];
    int32_t nd = 0;
    EXPECT(cm_convrnn_param_info(m, i, &name, shape, &nd) == 0 && nd == 4);
    const int64_t numel = shape[0] * shape[1] * shape[2] * shape[3];
    std::vector<float> w((size_t)numel), back((size_t)numel);
    for (size_t k = 0; k < w.size(); ++k) w[k] = wval(i, k);
    EXPECT(cm_convrnn_set_param(m, name, w.data(), numel - 1) != 0);
    EXPECT(cm_convrnn_set_param(m, name, w.data(), numel) == 0);
    EXPECT(cm_convrnn_get_param(m, name, back.data(), numel) == 0 && back == w);
  }
  const char *name = nullptr;
  int64_t shape[4];
  int32_t nd = 0;
  EXPECT(cm_convrnn_param_info(m, n, &name, shape, &nd) != 0);
  float one = 0.f;
  EXPECT(cm_convrnn_set_param(m, "encoder.encoder_cell_list.9.weight", &one, 1) != 0);
  EXPECT(cm_convrnn_finalize(m) != 0 && strstr(cm_last_error(), "host-only"));
  EXPECT(cm_convrnn_forecast_host(m, &one, &one, 0, 0, &one, 1) != 0);
  double fl = 0, by = 0;
  EXPECT(cm_convrnn_cost(m, 2, &fl, &by) == 0 && fl > 0 && by > 0);

  // the precision rules: fp32 or f16, before finalize; the f16 plan is inference only and its weights are two bytes
  double fl16 = 0, by16 = 0;
  EXPECT(cm_convrnn_set_precision(m, CM_PRECISION_F32R) != 0 && cm_convrnn_set_precision(m, CM_PRECISION_F32X) != 0);
  EXPECT(cm_convrnn_set_precision(m, 9) != 0 && strstr(cm_last_error(), "unknown precision"));
  EXPECT(cm_convrnn_set_precision(m, CM_PRECISION_F16) == 0 && m->precision == CM_PRECISION_F16);
  EXPECT(cm_convrnn_cost(m, 2, &fl16, &by16) == 0 && fl16 == fl && by16 < by);
  EXPECT(cm_convrnn_train_init(m, 1e-3f, 0.9f, 0.999f, 1e-8f, 0.f) != 0 && strstr(cm_last_error(), "inference only"));
  double sums16[6];
  EXPECT(cm_convrnn_loss_sums(m, &one, &one, 0, 1, nullptr, sums16) != 0 && strstr(cm_last_error(), "inference only"));
  EXPECT(cm_convrnn_debug_launch(m, 1, 0, &one, &one, &one, nullptr, nullptr, &one, &one, 1) != 0);   // not finalized
  EXPECT(cm_convrnn_set_precision(m, CM_PRECISION_F32) == 0 && m->precision == CM_PRECISION_F32);

  // the packers, element by element
  std::vector<float> w0, w1;
  for (int i = 0; i < 13; ++i) {
    const CrnnLayer &l = m->L[i];
    crnn_pack_layer(m, i, &w0, &w1);
    const Param *p = &m->params[l.p0];
    if (l.kind == CRNN_UP) {
      EXPECT(w0.size() == (size_t)16 * l.cin * l.cout && w1.empty());
      for (int cls = 0; cls < 4; ++cls)
        for (int nn = 0; nn < l.cout; ++nn)
          for (int tap = 0; tap < 4; ++tap)
            for (int ch = 0; ch < l.cin; ++ch) {
              const int ky = 1 - (cls >> 1) + 2 * (tap >> 1), kx = 1 - (cls & 1) + 2 * (tap & 1);
              // the tap's output row 2 iy - 1 + ky has the parity of the class, and input row iy = qy + py - ty
              EXPECT(((ky + 1) & 1) == (cls >> 1) && ((kx + 1) & 1) == (cls & 1));
              if (w0[(((size_t)cls * l.cout + nn) * 4 + tap) * l.cin + ch] != p->host[(((size_t)ch * l.cout + nn) * 4 + ky) * 4 + kx]) { fprintf(stderr, "transposed pack differs in layer %d\n", i); ++failures; return; }
            }
      continue;
    }
    const bool cellk = l.kind == CRNN_CELL, gru = cell == CM_CELL_GRU;
    const int cin = cellk ? l.cin + l.cout : l.cin, cpad = (cin + 7) / 8 * 8;
    const int N = cellk ? (gru ? 2 : 4) * l.cout : l.cout;
    EXPECT(w0.size() == (size_t)N * 9 * cpad);
    EXPECT(w1.size() == (cellk && gru ? (size_t)l.cout * 9 * cpad : 0));
    for (int row = 0; row < N; ++row)
      for (int t = 0; t < 9; ++t)
        for (int ch = 0; ch < cpad; ++ch) {
          float want = 0.f;
          if (ch < cin) {
            const Param *src = p;
            int n_src = row;
            if (cellk && gru) { src = p + row / l.cout; n_src = row % l.cout; }          // reset rows, then update rows
            if (cellk && !gru) n_src = (row % 4) * l.cout + row / 4;                       // packed row 4 ch + gate
            want = src->host[((size_t)n_src * cin + ch) * 9 + t];
          }
          if (w0[(size_t)row * 9 * cpad + (size_t)t * cpad + ch] != want) { fprintf(stderr, "3x3 pack differs in layer %d\n", i); ++failures; return; }
        }
    if (cellk && gru)
      for (int row = 0; row < l.cout; ++row)
        for (int t = 0; t < 9; ++t)
          for (int ch = 0; ch < cin; ++ch)
            if (w1[(size_t)row * 9 * cin + (size_t)t * cin + ch] != p[2].host[((size_t)row * cin + ch) * 9 + t]) { fprintf(stderr, "candidate pack differs in layer %d\n", i); ++failures; return; }
  }
  test_train_packs(m, cell);
  EXPECT(cm_convrnn_train_init(m, 1e-3f, 0.9f, 0.999f, 1e-8f, 0.f) != 0 && strstr(cm_last_error(), "host-only"));
  double terms[4];
  EXPECT(cm_convrnn_loss(m, &one, &one, 0, 1e-6, terms, 1, nullptr) != 0 && strstr(cm_last_error(), "host-only"));
  EXPECT(cm_convrnn_train_step(m, &one, &one, 0, 1e-6, 1.0, terms, 1, 1, nullptr) != 0 && strstr(cm_last_error(), "host-only"));
  EXPECT(cm_convrnn_train_sync(m) != 0 && cm_convrnn_train_get_grad(m, "x", &one, 1) != 0);
  // the split step
  double sums[6] = {1.5, 2.0, 1.0, 3.0, 2.0, 3.0};
  float *gp = nullptr;
  int64_t gn = 0;
  EXPECT(cm_convrnn_train_forward(m, &one, &one, 0, 1, nullptr, sums) != 0 && strstr(cm_last_error(), "host-only"));
  EXPECT(cm_convrnn_loss_sums(m, &one, &one, 0, 1, nullptr, sums) != 0 && strstr(cm_last_error(), "host-only"));
  EXPECT(cm_convrnn_train_backward(m, sums, 1e-6, 1.0, terms, nullptr) != 0 && strstr(cm_last_error(), "host-only"));
  EXPECT(cm_convrnn_train_flat_grads(m, &gp, &gn) != 0 && strstr(cm_last_error(), "host-only"));
  EXPECT(cm_convrnn_loss_terms_from_sums(sums, 0.0, terms) == 0 && terms[0] == 0.5 && terms[2] == 2.0 && terms[3] == 1.5 && terms[1] == 3.5);
  EXPECT(cm_convrnn_loss_terms_from_sums(nullptr, 0.0, terms) != 0);
  sums[5] = 0;
  EXPECT(cm_convrnn_loss_terms_from_sums(sums, 0.0, terms) != 0 && strstr(cm_last_error(), "element count"));
  EXPECT(cm_convrnn_destroy(m) == 0);
}

}  // namespace

int main() {
  test_handle(CM_CELL_GRU);
  test_handle(CM_CELL_LSTM);
  refused([](cm_convrnn_config &c) { c.in_channels = 3; }, "in_channels must be 4");
  refused([](cm_convrnn_config &c) { c.rows = 10; }, "multiples of 4");
  refused([](cm_convrnn_config &c) { c.cols = 0; }, "multiples of 4");
  refused([](cm_convrnn_config &c) { c.enc_kernels[2] = 5; }, "enc_kernels must be [3,3,3,3,3,3]");
  refused([](cm_convrnn_config &c) { c.forc_kernels[1] = 3; }, "forc_kernels must be [3,4,3,4,3,3,3]");
  refused([](cm_convrnn_config &c) { c.enc_hidden[2] = 48; }, "enc_hidden[2] == enc_hidden[1]");
  refused([](cm_convrnn_config &c) { c.enc_hidden[4] = 80; }, "enc_hidden[4] == enc_hidden[3]");
  refused([](cm_convrnn_config &c) { c.forc_hidden[0] = 80; }, "forc_hidden[0] == enc_hidden[5]");
  refused([](cm_convrnn_config &c) { c.forc_hidden[1] = 80; }, "forc_hidden[1] == enc_hidden[5]");
  refused([](cm_convrnn_config &c) { c.forc_hidden[3] = 80; }, "forc_hidden[3] == enc_hidden[3]");
  refused([](cm_convrnn_config &c) { c.forc_hidden[5] = 48; }, "forc_hidden[5] == enc_hidden[1]");
  refused([](cm_convrnn_config &c) { c.past_len = 0; }, "past_len must be >= 1");
  refused([](cm_convrnn_config &c) { c.future_len = 0; }, "future_len must be >= 1");
  refused([](cm_convrnn_config &c) { c.enc_hidden[0] = 12; }, "multiples of 8");
  refused([](cm_convrnn_config &c) { c.forc_hidden[6] = 1032; }, "multiples of 8 in [8, 1024]");
  refused([](cm_convrnn_config &c) { c.cell = 2; }, "cell must be");
  refused([](cm_convrnn_config &c) { c.max_batch = 0; }, "max_batch");
  refused([](cm_convrnn_config &c) { c.max_batch = 1 << 24; }, "2^31 - 64");
  {   // 256-channel layers are admitted
    cm_convrnn_config c = base_cfg(CM_CELL_LSTM);
    for (int i = 0; i < 6; ++i) c.enc_hidden[i] = 256;
    for (int i = 0; i < 7; ++i) c.forc_hidden[i] = 256;
    cm_convrnn *h = nullptr;
    EXPECT(cm_convrnn_create(&c, &h) == 0);
    cm_convrnn_destroy(h);
  }
  if (failures) { fprintf(stderr, "%d failure(s)\n", failures); return 1; }
  printf("convrnn selftest ok\n");
  return 0;
}
