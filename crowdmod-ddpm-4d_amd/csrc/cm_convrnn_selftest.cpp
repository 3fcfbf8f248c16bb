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
