// Host-side self-test of libcrowdmod_hip's C++ (`make asan`): the plan builder, the weight / index
// packers, the tile planner with its coordinate tables, the schedule and the error paths, compiled
// under AddressSanitizer + UBSan and run WITHOUT a GPU ("sanitizers": GPU ASan is
// not available on this pool, so the pointer-heavy host code is what gets sanitised).  It includes
// cm_model.cpp itself to reach the internal functions; no kernel is ever launched.
#include "cm_model.cpp"

#include <cstdlib>
#include <limits>
#include <random>

namespace {

int g_checks = 0;
#define EXPECT(cond)                                                                  \
  do {                                                                                \
    ++g_checks;                                                                       \
    if (!(cond)) { fprintf(stderr, "selftest FAILED: %s (%s:%d)\n", #cond, __FILE__, __LINE__); exit(1); } \
  } while (0)

void test_schedule() {
  for (int T : {2, 3, 50, 1000}) {
    cm_schedule *s = nullptr;
    EXPECT(cm_schedule_create(T, 0.5f, 1e-4f, 2e-2f, -1, &s) == 0);
    std::vector<float> buf((size_t)T);
    for (int w = 0; w < 6; ++w) EXPECT(cm_schedule_table(s, w, buf.data(), T) == 0);
    EXPECT(cm_schedule_table(s, 6, buf.data(), T) != 0);
    EXPECT(cm_schedule_table(s, 0, buf.data(), T - 1) != 0);
    cm_sample_opts o{};
    int32_t n = 0;
    o.sampler = CM_SAMPLER_DDPM;
    EXPECT(cm_sample_num_steps(s, &o, &n) == 0 && n == T);
    for (int d : {1, 2, 7, 100, 5000}) {
      o.sampler = CM_SAMPLER_DDIM; o.ddim_divider = d;
      EXPECT(cm_sample_num_steps(s, &o, &n) == 0 && n == (T - 1 + d - 1) / d);
    }
    o.sampler = CM_SAMPLER_FM_EULER; o.fm_steps = 10; o.fm_time_max_pos = 1000;
    EXPECT(cm_sample_num_steps(s, &o, &n) == 0 && n == 10);
    o.first_steps = 3;
    EXPECT(cm_sample_num_steps(s, &o, &n) == 0 && n == 3);
    // a host-only schedule must refuse device work instead of dereferencing null tables
    EXPECT(cm_q_sample(s, buf.data(), (const int64_t *)buf.data(), buf.data(), buf.data(), 1, 1, nullptr) != 0);
    EXPECT(cm_schedule_destroy(s) == 0);
  }
  cm_schedule *s = nullptr;
  EXPECT(cm_schedule_create(1, 0.5f, 1e-4f, 2e-2f, -1, &s) != 0);
  EXPECT(cm_schedule_create(10, 0.5f, 1e-4f, 2e-2f, -1, nullptr) != 0);
}

cm_unet_config atc_cfg(int C, int rows, int cols, int device) {
  cm_unet_config c{};
  c.in_channels = c.out_channels = C;
  c.num_res_blocks = 1; c.base_channels = 32; c.n_levels = 3;
  const int mult[3] = {1, 2, 4}, att[3] = {0, 0, 1};
  for (int i = 0; i < 3; ++i) { c.channel_mult[i] = mult[i]; c.apply_attention[i] = att[i]; }
  c.time_multiple = 4; c.rows = rows; c.cols = cols; c.past_len = 5; c.future_len = 3; c.max_batch = 2; c.device = device;
  return c;
}

void test_plan_and_params() {
  std::mt19937 rng(1);
  std::uniform_real_distribution<float> U(-1.f, 1.f);
  for (int C : {3, 4}) {
    cm_unet_config c = atc_cfg(C, 12, 36, -1);
    cm_model *m = nullptr;
    EXPECT(cm_model_create(&c, &m) == 0);
    int32_t n = 0;
    EXPECT(cm_model_num_params(m, &n) == 0 && n == 169);
    for (int i = 0; i < n; ++i) {
      const char *name = nullptr; int64_t shape[5]; int32_t nd = 0;
      EXPECT(cm_model_param_info(m, i, &name, shape, &nd) == 0 && name && nd >= 1 && nd <= 5);
      int64_t numel = 1;
      for (int d = 0; d < nd; ++d) numel *= shape[d];
      std::vector<float> w((size_t)numel), back((size_t)numel);
      for (auto &v : w) v = U(rng);
      EXPECT(cm_model_set_param(m, name, w.data(), numel) == 0);
      EXPECT(cm_model_set_param(m, name, w.data(), numel + 1) != 0);
      EXPECT(cm_model_get_param(m, name, back.data(), numel) == 0 && back == w);
    }
    EXPECT(cm_model_param_info(m, n, nullptr, nullptr, nullptr) != 0);
    EXPECT(cm_model_set_param(m, "no.such.tensor", (const float *)&n, 1) != 0);
    EXPECT(cm_model_finalize(m) != 0);                     // host-only: no CPU path
    EXPECT(std::string(cm_last_error()).find("host-only") != std::string::npos);
    EXPECT(cm_unet_forward(m, nullptr, nullptr, nullptr, nullptr, 1, nullptr) != 0);
    EXPECT(cm_model_destroy(m) == 0);
  }
  cm_unet_config bad = atc_cfg(3, 12, 36, -1);
  cm_model *m = nullptr;
  bad.base_channels = 12; EXPECT(cm_model_create(&bad, &m) != 0);
  bad = atc_cfg(3, 12, 36, -1); bad.n_levels = 9; EXPECT(cm_model_create(&bad, &m) != 0);
  bad = atc_cfg(9, 12, 36, -1); EXPECT(cm_model_create(&bad, &m) != 0);
  bad = atc_cfg(3, 12, 36, -1); bad.max_batch = 0; EXPECT(cm_model_create(&bad, &m) != 0);
  EXPECT(cm_model_create(nullptr, &m) != 0);
}

// fragment element i holds source element idx[i], or the zero padding where idx[i] is -1
void expect_gather(const std::vector<float> &frag, const std::vector<int> &idx, const std::vector<float> &src) {
  EXPECT(frag.size() == idx.size());
  for (size_t i = 0; i < idx.size(); ++i) {
    EXPECT(idx[i] >= -1 && idx[i] < (int)src.size());
    if (idx[i] >= 0) EXPECT(frag[i] == src[(size_t)idx[i]]); else EXPECT(frag[i] == 0.f);
  }
}

// ---- fragment digests ------------------------------------------------------------------------------------------------------------
// Every packer's output bytes on fixed inputs, as 64-bit FNV-1a digests recorded from the packers as they stood before the layouts moved
// to cm_pack.h: a refactor of a layout must leave every fragment bit for bit what it was.
uint64_t fnv1a(const void *p, size_t n, uint64_t h = 0xcbf29ce484222325ull) {
  const unsigned char *b = static_cast<const unsigned char *>(p);
  for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 0x100000001b3ull; }
  return h;
}
template <class T>
uint64_t digest(const std::vector<T> &v, long long extra = 0) {
  return fnv1a(&extra, sizeof extra, fnv1a(v.data(), v.size() * sizeof(T)));
}
// Weights built from raw generator words by integer arithmetic alone (no library distribution): a full 24-bit significand (23 random
// fraction bits), both signs, magnitudes over eight binades [2^-4, 2^4) -- so a changed summation order, or a fold in float instead of
// double, changes a digest.
std::vector<float> digest_weights(std::mt19937 &rng, size_t n) {
  std::vector<float> w(n);
  for (auto &v : w) {
    const uint32_t r = rng();
    const uint32_t u = (r & 0x80000000u) | ((123u + ((r >> 24) & 7u)) << 23) | (r & 0x7fffffu);
    std::memcpy(&v, &u, 4);
  }
  return w;
}

struct Digest { std::string name; uint64_t d; };

std::vector<Digest> fragment_digests() {
  std::vector<Digest> out;
  std::mt19937 rng(20260);
  auto tag = [](const char *what, std::initializer_list<int> dims) {
    std::string s = what;
    for (int d : dims) s += "_" + std::to_string(d);
    return s;
  };
  // generic layout, and its f16 flavour on the base, three-chunk and one-parity-class cases
  struct Gen { int Co, Ci, ntaps, Ci_pad, CK, NB; bool f16; };
  const Gen gens[] = {{32, 32, 27, 32, 32, 1, true},   {40, 24, 27, 24, 8, 2, false},   {32, 3, 27, 8, 8, 1, false},
                      {64, 96, 27, 96, 32, 2, true},   {128, 192, 1, 192, 64, 2, false}, {64, 64, 8, 64, 32, 2, true}};
  for (const Gen &c : gens) {
    const std::vector<float> W = digest_weights(rng, (size_t)c.Co * c.Ci * c.ntaps);
    // (8 taps: one parity class, already in its own e order)
    const std::vector<float> wi = c.ntaps == 8 ? W : to_internal_taps(W.data(), c.Co, c.Ci, c.ntaps);
    out.push_back({tag("taps", {c.Co, c.Ci, c.ntaps}), digest(wi)});
    out.push_back({tag("conv", {c.Co, c.Ci, c.ntaps, c.Ci_pad, c.CK, c.NB}), digest(pack_conv(wi.data(), c.Co, c.Ci, c.ntaps, c.Ci_pad, c.CK, c.NB))});
    if (c.f16)
      out.push_back({tag("conv_f16", {c.Co, c.Ci, c.ntaps, c.Ci_pad, c.CK, c.NB}), digest(pack_conv_f16(wi.data(), c.Co, c.Ci, c.ntaps, c.Ci_pad, c.CK, c.NB))});
  }
  // parity fold + the 8-class concatenation through each per-class packer
  for (auto cc : {std::make_pair(32, 32), std::make_pair(64, 96)}) {
    const int Co = cc.first, Ci = cc.second, NB = Co > 32 ? 2 : 1;
    const std::vector<float> W = digest_weights(rng, (size_t)Co * Ci * 27);
    const std::vector<float> wp = parity_weights(to_internal_taps(W.data(), Co, Ci, 27), Co, Ci);
    out.push_back({tag("parity", {Co, Ci}), digest(wp)});
    const float ws = h2_wscale(wp.data(), wp.size());
    EXPECT(ws > 0.f);
    long long stride = 0;
    const std::vector<float> g = pack_parity_classes(wp, &stride, [&](const float *w8) { return pack_conv(w8, Co, Ci, 8, Ci, 32, NB); });
    out.push_back({tag("parity_conv", {Co, Ci}), digest(g, stride)});
    const std::vector<float> b6 = pack_parity_classes(wp, &stride, [&](const float *w8) { return pack_ups_b6(w8, Co, Ci); });
    out.push_back({tag("parity_ups_b6", {Co, Ci}), digest(b6, stride)});
    const std::vector<float> h2 = pack_parity_classes(wp, &stride, [&](const float *w8) { return pack_ups_b6(w8, Co, Ci, ws); });
    out.push_back({tag("parity_ups_h2", {Co, Ci}), digest(h2, stride)});
    const std::vector<float> f16 = pack_parity_classes(wp, &stride, [&](const float *w8) { return pack_ups_f16(w8, Co, Ci); });
    out.push_back({tag("parity_ups_f16", {Co, Ci}), digest(f16, stride)});
  }
  // whole-sample quarter-resolution kernel: (32, 16) has the padded 16-channel step (2 channels per wave)
  for (auto cc : {std::make_pair(32, 16), std::make_pair(64, 64), std::make_pair(128, 192)}) {
    const int Co = cc.first, Ci = cc.second;
    const std::vector<float> wi = digest_weights(rng, (size_t)Co * Ci * 27), w2 = digest_weights(rng, (size_t)Co * Ci);
    const std::vector<float> wq = pack_qr(wi, Co, Ci);
    out.push_back({tag("qr", {Co, Ci}), digest(wq)});
    out.push_back({tag("qr_b6", {Co, Ci}), digest(pack_qr_b6(wq, Co, Ci))});
    out.push_back({tag("qr_h2", {Co, Ci}), digest(pack_qr_b6(wq, Co, Ci, h2_wscale(wq.data(), wq.size())))});
    out.push_back({tag("qr_skip", {Co, Ci}), digest(pack_qr_skip(w2.data(), Co, Ci))});
  }
  // first conv (Co = 32): 3 and 4 of 4 input channels, 5 and 8 of 8
  for (int Ci : {3, 4, 5, 8}) {
    const std::vector<float> wi = digest_weights(rng, (size_t)32 * Ci * 27);
    out.push_back({tag("first", {32, Ci}), digest(pack_first(wi.data(), 32, Ci, Ci <= 4 ? 4 : 8))});
  }
  // small-N last conv: 3 and 4 of 4 output channels, 5 and 8 of 8; 3 of 8 padded input channels
  for (int Co : {3, 4, 5, 8}) {
    const std::vector<float> wi = digest_weights(rng, (size_t)Co * 32 * 27);
    out.push_back({tag("small", {Co, 32, 32, 32}), digest(pack_small(wi.data(), Co, 32, 32, 32, Co <= 4 ? 4 : 8))});
  }
  {
    const std::vector<float> wi = digest_weights(rng, (size_t)3 * 3 * 27);
    out.push_back({tag("small", {3, 3, 8, 8}), digest(pack_small(wi.data(), 3, 3, 8, 8, 4))});
  }
  // Winograd: fp32, f16, six-term and h2
  for (auto cc : {std::make_pair(32, 16), std::make_pair(64, 96)}) {
    const int Co = cc.first, Ci = cc.second;
    const std::vector<float> wi = digest_weights(rng, (size_t)Co * Ci * 27);
    const std::vector<float> ww = pack_wino(wi, Co, Ci, Ci);
    out.push_back({tag("wino", {Co, Ci}), digest(ww)});
    out.push_back({tag("wino_f16", {Co, Ci}), digest(pack_wino_f16(wi, Co, Ci, Ci))});
    out.push_back({tag("wino_b6", {Co, Ci}), digest(pack_wino_b6(ww))});
    out.push_back({tag("wino_h2", {Co, Ci}), digest(pack_wino_b6(ww, h2_wscale(ww.data(), ww.size())))});
  }
  // f16 plan: direct kernel, 1x1x1 (96 of 128 output channels in the second tile)
  {
    const std::vector<float> wi = digest_weights(rng, (size_t)64 * 32 * 27), w1 = digest_weights(rng, (size_t)96 * 32);
    for (int NB : {1, 2}) out.push_back({tag("f16d", {64, 32, 27, NB}), digest(pack_f16d(wi.data(), 64, 32, 27, NB))});
    for (int NB : {1, 2}) out.push_back({tag("1x1_f16", {96, 32, NB}), digest(pack_1x1_f16(w1.data(), 96, 32, NB))});
  }
  // whole-sample attention kernel
  for (auto nk : {std::make_pair(48, 32), std::make_pair(128, 128)}) {
    const std::vector<float> w = digest_weights(rng, (size_t)nk.first * nk.second);
    out.push_back({tag("attn_h2", {nk.first, nk.second}), digest(pack_attn_h2(w.data(), nk.first, nk.second, h2_wscale(w.data(), w.size())))});
  }
  // the whole h2 helper (scale + fragments) from a reference-layout weight; all-zero weights and weights with one infinity have no
  // scale and get no fragments
  struct H2 { H2Kind kind; const char *name; int Co, Ci; };
  const H2 h2s[] = {{H2_FIN, "h2_fin", 3, 32}, {H2_WINO, "h2_wino", 64, 96}, {H2_QR, "h2_qr", 64, 64}, {H2_UPS, "h2_ups", 32, 32}};
  for (const H2 &c : h2s) {
    std::vector<float> w = digest_weights(rng, (size_t)c.Co * c.Ci * 27), frag;
    const float ws = h2_fragments(c.kind, w.data(), c.Co, c.Ci, &frag);
    EXPECT(ws > 0.f && (c.kind == H2_FIN) == frag.empty());
    long long ws_bits = 0;
    std::memcpy(&ws_bits, &ws, 4);
    out.push_back({tag(c.name, {c.Co, c.Ci}), digest(frag, ws_bits)});
    frag.clear();
    w[w.size() / 3] = std::numeric_limits<float>::infinity();
    EXPECT(h2_fragments(c.kind, w.data(), c.Co, c.Ci, &frag) == 0.f && frag.empty());
    std::fill(w.begin(), w.end(), 0.f);
    EXPECT(h2_fragments(c.kind, w.data(), c.Co, c.Ci, &frag) == 0.f && frag.empty());
  }
  return out;
}

void test_fragment_digests() {
  static const struct { const char *name; uint64_t d; } want[] = {
      {"taps_32_32_27", 0x820a5de693853861ull},
      {"conv_32_32_27_32_32_1", 0xfbc284684e8b9771ull},
      {"conv_f16_32_32_27_32_32_1", 0x22bfedb98083e5d7ull},
      {"taps_40_24_27", 0x3008ce9498a90dd8ull},
      {"conv_40_24_27_24_8_2", 0xf34a22de97258540ull},
      {"taps_32_3_27", 0x2fa3ac24aa9974e8ull},
      {"conv_32_3_27_8_8_1", 0xd52e2501401ccc70ull},
      {"taps_64_96_27", 0xde6d731ca3c825f5ull},
      {"conv_64_96_27_96_32_2", 0x4c42cbe1a7d7d469ull},
      {"conv_f16_64_96_27_96_32_2", 0xb4d5fafb0c4f0fceull},
      {"taps_128_192_1", 0x67bbf4fd37aa7a2dull},
      {"conv_128_192_1_192_64_2", 0xafa843c6b6359db1ull},
      {"taps_64_64_8", 0x778dd0a9b8267264ull},
      {"conv_64_64_8_64_32_2", 0x0b2d450649c17bfcull},
      {"conv_f16_64_64_8_64_32_2", 0xf6bb147c91004590ull},
      {"parity_32_32", 0x42dbd1be1df39487ull},
      {"parity_conv_32_32", 0xa5b8ec34ad30ad4bull},
      {"parity_ups_b6_32_32", 0x5b7d83fc367af890ull},
      {"parity_ups_h2_32_32", 0x30faf7615c981d88ull},
      {"parity_ups_f16_32_32", 0xd394af8fa3c998b6ull},
      {"parity_64_96", 0xc4b58d87886dc5d9ull},
      {"parity_conv_64_96", 0x8193d7884570537dull},
      {"parity_ups_b6_64_96", 0x09a99acba4c69f68ull},
      {"parity_ups_h2_64_96", 0x038a11f5b1f6e67eull},
      {"parity_ups_f16_64_96", 0xe3fa39dc94e2b1a9ull},
      {"qr_32_16", 0x58412134865cfbf6ull},
      {"qr_b6_32_16", 0x0ef963b4b36a00e9ull},
      {"qr_h2_32_16", 0x075325de759b7942ull},
      {"qr_skip_32_16", 0xa1d0aa697ee6ea36ull},
      {"qr_64_64", 0xa490111431f27e05ull},
      {"qr_b6_64_64", 0x402032d474195320ull},
      {"qr_h2_64_64", 0x43b749f659ceac49ull},
      {"qr_skip_64_64", 0xd8a30f37caf41c6cull},
      {"qr_128_192", 0x051db83360196265ull},
      {"qr_b6_128_192", 0x0e53e1d8ad010f43ull},
      {"qr_h2_128_192", 0xaba34ab55ac37a0dull},
      {"qr_skip_128_192", 0x1f49c64dae5c1eb6ull},
      {"first_32_3", 0x85e622c61b8ea8beull},
      {"first_32_4", 0x14dde78bee8b9713ull},
      {"first_32_5", 0xe0048aca83c63c7cull},
      {"first_32_8", 0x1b31c6efd1f9199dull},
      {"small_3_32_32_32", 0x82f64ac22f6431c8ull},
      {"small_4_32_32_32", 0x7faa7f1290d32e13ull},
      {"small_5_32_32_32", 0xd6bd6fb6ed697861ull},
      {"small_8_32_32_32", 0xb6fca231c0852828ull},
      {"small_3_3_8_8", 0xd9507e0d72aee490ull},
      {"wino_32_16", 0xe60e5c814351dbf7ull},
      {"wino_f16_32_16", 0x30db97b589846670ull},
      {"wino_b6_32_16", 0x03be74e468ffd285ull},
      {"wino_h2_32_16", 0x35026faa11129b4dull},
      {"wino_64_96", 0x13c797f5d6645704ull},
      {"wino_f16_64_96", 0x547b13a77069a2bbull},
      {"wino_b6_64_96", 0x614bdcfacf53fdacull},
      {"wino_h2_64_96", 0xeccc0c63cc596680ull},
      {"f16d_64_32_27_1", 0x45dd1faefb431eb9ull},
      {"f16d_64_32_27_2", 0x32f04be83c18b49dull},
      {"1x1_f16_96_32_1", 0x6fe1fa8106ae219dull},
      {"1x1_f16_96_32_2", 0x6e31becb0d7be2c5ull},
      {"attn_h2_48_32", 0xe991c10c27ae644aull},
      {"attn_h2_128_128", 0x5a7f2dfc5cdbe892ull},
      {"h2_fin_3_32", 0xa1c5362786b728f9ull},
      {"h2_wino_64_96", 0xc4e14f6f365d2323ull},
      {"h2_qr_64_64", 0x613cd27fece883f3ull},
      {"h2_ups_32_32", 0xbf8bbe9249def9eeull},
  };
  const std::vector<Digest> got = fragment_digests();
  EXPECT(got.size() == sizeof want / sizeof want[0]);
  for (size_t i = 0; i < got.size(); ++i) {
    if (got[i].name != want[i].name || got[i].d != want[i].d)
      fprintf(stderr, "fragment digest %zu: %s 0x%016llx, recorded %s 0x%016llx\n", i, got[i].name.c_str(), (unsigned long long)got[i].d,
              want[i].name, (unsigned long long)want[i].d);
    EXPECT(got[i].name == want[i].name && got[i].d == want[i].d);
  }
}

void test_packers() {
  std::mt19937 rng(2);
  std::uniform_real_distribution<float> U(-1.f, 1.f);
  struct Case { int Co, Ci, ntaps, Ci_pad, CK, NB; };
  const Case cases[] = {{32, 32, 27, 32, 32, 1}, {64, 96, 27, 96, 32, 2}, {32, 3, 27, 8, 8, 1}, {4, 32, 27, 32, 32, 1},
                        {384, 128, 1, 128, 128, 2}, {128, 192, 1, 192, 64, 2}, {40, 24, 27, 24, 8, 2}};
  for (const Case &c : cases) {
    std::vector<float> W((size_t)c.Co * c.Ci * c.ntaps);
    for (auto &v : W) v = U(rng);
    const std::vector<float> wi = to_internal_taps(W.data(), c.Co, c.Ci, c.ntaps);
    EXPECT(wi.size() == W.size());
    const std::vector<float> wf = pack_conv(wi.data(), c.Co, c.Ci, c.ntaps, c.Ci_pad, c.CK, c.NB);
    const int TN = 32 * c.NB, ntn = (c.Co + TN - 1) / TN;
    EXPECT(wf.size() == (size_t)ntn * (c.Ci_pad / c.CK) * c.ntaps * (c.CK / 8) * c.NB * 256);
    // every reference weight appears exactly once; everything else is zero padding
    double sa = 0, sb = 0;
    for (float v : wi) sa += std::fabs(v);
    for (float v : wf) sb += std::fabs(v);
    EXPECT(std::fabs(sa - sb) <= 1e-6 * sa + 1e-9);
    if (c.ntaps == 27) {
      const std::vector<float> wp = parity_weights(wi, c.Co, c.Ci);
      EXPECT(wp.size() == (size_t)8 * c.Co * c.Ci * 8);
      // each parity class redistributes all 27 taps: the tap sum per (co, ci) is preserved
      for (int p = 0; p < 8; ++p) {
        double s27 = 0, s8 = 0;
        for (int t = 0; t < 27; ++t) s27 += wi[t];
        for (int e = 0; e < 8; ++e) s8 += wp[(size_t)p * c.Co * c.Ci * 8 + e];
        EXPECT(std::fabs(s27 - s8) < 1e-5);
      }
    }
    // index version (training re-pack): same positions are filled
    std::vector<int> src((size_t)c.Co * c.Ci * c.ntaps);
    for (size_t i = 0; i < src.size(); ++i) src[i] = (int)i;
    const std::vector<int> pi = pack_conv(src.data(), c.Co, c.Ci, c.ntaps, c.Ci_pad, c.CK, c.NB, -1);
    expect_gather(wf, pi, wi);
  }
}

// Values against indices, for every layout that is packed as values when a handle loads and as indices for the re-pack after an
// optimizer step: the one template, on the positions 0, 1, 2, ... of the source, must name for every fragment element the source
// element the value packer put there.
void test_value_index_layouts() {
  std::mt19937 rng(7);
  auto iota_of = [](size_t n) { std::vector<int> v(n); std::iota(v.begin(), v.end(), 0); return v; };
  // quarter-resolution kernel and its fused skip; the data gradient packs W'[ci][co][flipped tap] with Co and Ci swapped
  for (auto cc : {std::make_pair(32, 16), std::make_pair(64, 64), std::make_pair(128, 192), std::make_pair(64, 128)}) {
    const int Co = cc.first, Ci = cc.second;
    const std::vector<float> wi = digest_weights(rng, (size_t)Co * Ci * 27), w2 = digest_weights(rng, (size_t)Co * Ci);
    expect_gather(pack_qr(wi, Co, Ci), pack_qr(iota_of(wi.size()), Co, Ci), wi);
    expect_gather(pack_qr_skip(w2.data(), Co, Ci), pack_qr_skip(iota_of(w2.size()).data(), Co, Ci), w2);
    if (Ci % 32) continue;
    std::vector<int> src((size_t)Ci * Co * 27);                  // train_setup's data-gradient map
    std::vector<float> wt(src.size());
    for (int ci = 0; ci < Ci; ++ci)
      for (int co = 0; co < Co; ++co)
        for (int t = 0; t < 27; ++t) {
          src[((size_t)ci * Co + co) * 27 + t] = (int)(((size_t)co * Ci + ci) * 27 + (26 - t));
          wt[((size_t)ci * Co + co) * 27 + t] = wi[((size_t)co * Ci + ci) * 27 + (26 - t)];
        }
    expect_gather(pack_qr(wt, Ci, Co), pack_qr(src, Ci, Co), wi);
    expect_gather(pack_conv(wt.data(), Ci, Co, 27, Co, 32, Ci > 32 ? 2 : 1), pack_conv(src.data(), Ci, Co, 27, Co, 32, Ci > 32 ? 2 : 1, -1), wi);
  }
  // first conv: 3 / 4 of 4 input channels, 5 / 8 of 8
  for (int Ci : {3, 4, 5, 8}) {
    const std::vector<float> wi = digest_weights(rng, (size_t)32 * Ci * 27);
    const int cin = Ci <= 4 ? 4 : 8;
    expect_gather(pack_first(wi.data(), 32, Ci, cin), pack_first(iota_of(wi.size()).data(), 32, Ci, cin, -1), wi);
  }
  // small-N last conv: 3 / 4 of 4 output channels, 5 / 8 of 8; 3 of 8 padded input channels
  struct Small { int Co, Ci, Ci_pad, CK; };
  for (const Small &c : {Small{3, 32, 32, 32}, Small{4, 32, 32, 32}, Small{5, 32, 32, 32}, Small{8, 32, 32, 32}, Small{3, 3, 8, 8}}) {
    const std::vector<float> wi = digest_weights(rng, (size_t)c.Co * c.Ci * 27);
    const int nco = c.Co <= 4 ? 4 : 8;
    expect_gather(pack_small(wi.data(), c.Co, c.Ci, c.Ci_pad, c.CK, nco), pack_small(iota_of(wi.size()).data(), c.Co, c.Ci, c.Ci_pad, c.CK, nco, -1), wi);
  }
  // parity fold: the 8 indexed sources of an element, summed in double in list order and rounded once, are the value fold bit for
  // bit -- before and after the per-class packing
  for (auto cc : {std::make_pair(32, 32), std::make_pair(40, 24)}) {
    const int Co = cc.first, Ci = cc.second, NB = Co > 32 ? 2 : 1, CK = Ci % 32 ? 8 : 32;
    const std::vector<float> wi = digest_weights(rng, (size_t)Co * Ci * 27);
    const std::vector<float> wp = parity_weights(wi, Co, Ci);
    const std::vector<Src8> sp = parity_sources(iota_of(wi.size()), Co, Ci);
    long long sv = 0, si = 0;
    const std::vector<float> fv = pack_parity_classes(wp, &sv, [&](const float *w8) { return pack_conv(w8, Co, Ci, 8, Ci, CK, NB); });
    const std::vector<Src8> fi = pack_parity_classes(sp, &si, [&](const Src8 *s8) { return pack_conv(s8, Co, Ci, 8, Ci, CK, NB, kNoSrc8); });
    EXPECT(sv == si && sv * 8 == (long long)fv.size());
    auto expect_fold = [&](const std::vector<float> &v, const std::vector<Src8> &idx) {
      EXPECT(v.size() == idx.size());
      for (size_t i = 0; i < v.size(); ++i) {
        double acc = 0;
        bool ended = false;
        for (int k = 0; k < 8; ++k) {
          const int j = idx[i][k];
          EXPECT(j >= -1 && j < (int)wi.size() && !(ended && j >= 0));   // (sources first, then -1s)
          if (j >= 0) acc += (double)wi[(size_t)j]; else ended = true;
        }
        const float folded = (float)acc;
        EXPECT(std::memcmp(&v[i], &folded, 4) == 0);
      }
    };
    expect_fold(wp, sp);
    expect_fold(fv, fi);
  }
}

void check_tables(const cm::ConvArgs &a, int MB) {
  const int HZ = (a.bz - 1) * a.stride + a.td, HY = (a.by - 1) * a.stride + a.td, HX = (a.bx - 1) * a.stride + a.td;
  const int hv = cm::conv_halo_voxels(a);
  EXPECT(hv == a.bs * HZ * HY * HX);
  std::vector<int> hvt((size_t)hv), mt((size_t)32 * MB);
  cm::conv_build_tables(a, MB, hvt.data(), mt.data());
  for (int v : hvt) {
    EXPECT((v & 511) < HX && ((v >> 9) & 511) < HY && ((v >> 18) & 255) < HZ && (v >> 26) < a.bs);
  }
  int valid = 0;
  for (int v : mt) {
    if (v < 0) continue;
    ++valid;
    EXPECT((v & 511) < a.bx && ((v >> 9) & 511) < a.by && ((v >> 18) & 255) < a.bz && (v >> 26) < a.bs);
  }
  EXPECT(valid == a.bs * a.bz * a.by * a.bx && valid <= 32 * MB);
  EXPECT(cm::conv_lds_bytes(a, MB, 1) > 0);
}

void test_tile_planner() {
  // every 3x3x3 / 1x1x1 layer shape of the three reference grids, through the same chooser the model uses
  struct Grid { int Z, Y, X; };
  const Grid grids[] = {{8, 12, 36}, {8, 28, 24}, {8, 24, 72}, {8, 4, 8}};
  for (const Grid &g : grids)
    for (int level = 0; level < 3; ++level)
      for (int ci : {32, 64, 128, 192, 256})
        for (int co : {32, 64, 128})
          for (int mode = 0; mode < 4; ++mode) {   // 0: 3x3x3 s1, 1: stride 2, 2: parity upsample, 3: 1x1x1
            Op op;
            op.kind = OP_CONV;
            cm::ConvArgs &a = op.ca;
            const int Z = g.Z >> level, Y = g.Y >> level, X = g.X >> level;
            if (Z < 1 || Y < 1 || X < 1) continue;
            if (mode == 1 && (Z < 2 || Y < 2 || X < 2)) continue;
            a.C0 = ci; a.C1 = 0; a.Co = co; a.CK = mode == 3 ? 64 : 32;
            if (ci % a.CK) continue;
            a.ntaps = mode == 3 ? 1 : (mode == 2 ? 8 : 27);
            a.td = mode == 3 ? 1 : (mode == 2 ? 2 : 3);
            a.stride = mode == 1 ? 2 : 1; a.par = mode == 2; a.ups = 0;
            a.Zs = Z; a.Ys = Y; a.Xs = X;
            const int os = mode == 2 ? 2 : 1;
            a.Zo = mode == 1 ? Z / 2 : Z * os; a.Yo = mode == 1 ? Y / 2 : Y * os; a.Xo = mode == 1 ? X / 2 : X * os;
            op.NB = co > 32 ? 2 : 1;
            static Act dummy;
            op.stat_act = &dummy;
            pick_tile(op, TUNE_BATCH);
            EXPECT(op.MB >= 1 && op.MB <= 8 && cm::conv_variant_exists(op.MB, op.NB));
            EXPECT(a.bs >= 1 && a.bz >= 1 && a.by >= 1 && a.bx >= 1);
            EXPECT(a.bs * a.bz * a.by * a.bx <= 32 * op.MB);
            EXPECT(a.ntz * a.bz >= a.Zo / os && a.nty * a.by >= a.Yo / os && a.ntx * a.bx >= a.Xo / os);
            EXPECT(cm::conv_lds_bytes(a, op.MB, op.NB) <= 160 * 1024);
            check_tables(a, op.MB);
          }
}

// round 3: packers and planners of the new kernels (whole-sample quarter-resolution kernel, direct f16 kernel)
void test_round3_packers() {
  std::mt19937 rng(5);
  std::uniform_real_distribution<float> U(-1.f, 1.f);
  for (int Co : {32, 64, 128})
    for (int Ci : {16, 64, 192}) {
      std::vector<float> wi((size_t)Co * Ci * 27);
      for (auto &v : wi) v = U(rng);
      // pack_qr: every weight appears exactly once, at the documented position
      const std::vector<float> q = pack_qr(wi, Co, Ci);
      EXPECT(q.size() == wi.size());
      const int ng = 9 * (Ci / 8);
      for (int probe = 0; probe < 200; ++probe) {
        const int co = (int)(rng() % Co), ci = (int)(rng() % Ci), dz = (int)(rng() % 3), dy = (int)(rng() % 3), dx = (int)(rng() % 3);
        const int nt = co / 32, g = (ci / 8) * 9 + dy * 3 + dx, lane = 32 * ((ci % 8) / 4) + co % 32, jj = ci % 4;
        EXPECT(q[((((size_t)nt * ng + g) * 3 + dz) * 64 + lane) * 4 + jj] == wi[((size_t)co * Ci + ci) * 27 + (dz * 3 + dy) * 3 + dx]);
      }
      std::vector<float> w2((size_t)Co * Ci);
      for (auto &v : w2) v = U(rng);
      const std::vector<float> qs = pack_qr_skip(w2.data(), Co, Ci);
      EXPECT(qs.size() == w2.size());
      for (int probe = 0; probe < 100; ++probe) {
        const int co = (int)(rng() % Co), ci = (int)(rng() % Ci);
        EXPECT(qs[(((size_t)(co / 32) * (Ci / 8) + ci / 8) * 64 + 32 * ((ci % 8) / 4) + co % 32) * 4 + ci % 4] == w2[(size_t)co * Ci + ci]);
      }
      // pack_f16d: two halves per float, [nt][c16][tap][nb][lane][8]
      for (int NB : {1, 2}) {
        if (Co % (32 * NB) || Ci % 16) continue;
        const std::vector<float> f = pack_f16d(wi.data(), Co, Ci, 27, NB);
        EXPECT(f.size() * 2 == wi.size());
        const uint16_t *h = reinterpret_cast<const uint16_t *>(f.data());
        for (int probe = 0; probe < 100; ++probe) {
          const int co = (int)(rng() % Co), ci = (int)(rng() % Ci), t = (int)(rng() % 27);
          const int nt = co / (32 * NB), nb = (co % (32 * NB)) / 32, c = ci / 16, lane = 32 * ((ci % 16) / 8) + co % 32, j = ci % 8;
          const size_t o = (((((size_t)nt * (Ci / 16) + c) * 27 + t) * NB + nb) * 64 + lane) * 8 + j;
          EXPECT(h[o] == f32_to_f16_bits(wi[((size_t)co * Ci + ci) * 27 + t]));
        }
      }
      // pack_ups_b6: hi + mid + lo reproduces every weight EXACTLY (8 + 8 + 8 mantissa bits), at the documented positions
      if (Ci % 32 == 0) {
        std::vector<float> w8((size_t)Co * Ci * 8);
        for (auto &v : w8) v = U(rng) * (rng() % 7 == 0 ? 1e-6f : 1.f);
        const std::vector<float> f = pack_ups_b6(w8.data(), Co, Ci);
        EXPECT(f.size() * 2 == w8.size() * 3);
        const uint16_t *h = reinterpret_cast<const uint16_t *>(f.data());
        for (int probe = 0; probe < 200; ++probe) {
          const int co = (int)(rng() % Co), ci = (int)(rng() % Ci), t = (int)(rng() % 8);
          const int cbk = co / 32, ch = ci / 32, mg = (ci % 32) / 16, lane = 32 * ((ci % 16) / 8) + co % 32, i = ci % 8;
          float sum = 0.f;
          for (int tm = 2; tm >= 0; --tm)
            sum += bf16_bits_to_f32(h[(((((((size_t)cbk * (Ci / 32) + ch) * 8 + t) * 2 + mg) * 3 + tm) * 64) + lane) * 8 + i]);
          EXPECT(sum == w8[((size_t)co * Ci + ci) * 8 + t]);
        }
      }
      // pack_ups_f16 (one parity class, [Co][Ci][8]): [column block][chunk][tap][16-channel group][lane][8]
      if (Ci % 32 == 0) {
        std::vector<float> w8((size_t)Co * Ci * 8);
        for (auto &v : w8) v = U(rng);
        const std::vector<float> f = pack_ups_f16(w8.data(), Co, Ci);
        EXPECT(f.size() * 2 == w8.size());
        const uint16_t *h = reinterpret_cast<const uint16_t *>(f.data());
        for (int probe = 0; probe < 100; ++probe) {
          const int co = (int)(rng() % Co), ci = (int)(rng() % Ci), t = (int)(rng() % 8);
          const int cbk = co / 32, ch = ci / 32, mg = (ci % 32) / 16, lane = 32 * ((ci % 16) / 8) + co % 32, i = ci % 8;
          const size_t o = ((((((size_t)cbk * (Ci / 32) + ch) * 8 + t) * 2 + mg) * 64) + lane) * 8 + i;
          EXPECT(h[o] == f32_to_f16_bits(w8[((size_t)co * Ci + ci) * 8 + t]));
        }
      }
    }
  // tile planner of the direct f16 kernel: every reference grid level gets a tile that divides it and fits the kernel's limits
  const int grids[][3] = {{8, 12, 36}, {4, 6, 18}, {8, 28, 24}, {4, 14, 12}, {8, 24, 72}, {4, 12, 36}};
  for (auto &g : grids) {
    int bz = 0, by = 0, bx = 0, mbw = 0;
    EXPECT(cm::conv_f16d_pick(g[0], g[1], g[2], &bz, &by, &bx, &mbw));
    EXPECT(g[0] % bz == 0 && g[1] % by == 0 && g[2] % bx == 0 && bz * by * bx <= 128 * mbw && mbw >= 1 && mbw <= 2);
    cm::ConvArgs a{};
    a.ntaps = 27; a.stride = 1; a.C0 = 32; a.Co = 32; a.Zs = a.Zo = g[0]; a.Ys = a.Yo = g[1]; a.Xs = a.Xo = g[2]; a.bz = bz; a.by = by; a.bx = bx;
    EXPECT(cm::conv_f16d_ok(a, mbw) && cm::conv_f16d_slots(a, mbw) <= MAX_SLOTS);
  }
  // stage-once upsample kernel: a source tile for every upsample source grid of the reference configs (ATC, CR-120, 24x72),
  // planes tiles where a plane fits one row block; the launcher's own feasibility test agrees with the picker
  const int srcs[][3] = {{2, 3, 9}, {4, 6, 18}, {2, 7, 6}, {4, 14, 12}, {2, 6, 18}, {4, 12, 36}};
  for (auto &g : srcs) {
    int tz = 0, ty = 0, tx = 0, mbw = 0, planes = 0;
    EXPECT(cm::conv_ups_pick(g[0], g[1], g[2], &tz, &ty, &tx, &mbw, &planes));
    EXPECT(g[0] % tz == 0 && g[1] % ty == 0 && g[2] % tx == 0 && mbw >= 1 && mbw <= 5 && (tz + 1) * (ty + 2) * (tx + 2) <= 320);
    EXPECT(planes ? (ty * tx <= 32 && mbw == tz) : tz * ty * tx <= 32 * mbw);
    cm::ConvArgs a{};
    a.par = 1; a.ntaps = 8; a.td = 2; a.CK = 32; a.C0 = 64; a.Co = 64; a.Zs = g[0]; a.Ys = g[1]; a.Xs = g[2];
    a.Zo = 2 * g[0]; a.Yo = 2 * g[1]; a.Xo = 2 * g[2]; a.bz = tz; a.by = ty; a.bx = tx; a.ntz = g[0] / tz; a.nty = g[1] / ty; a.ntx = g[2] / tx;
    EXPECT(cm::conv_ups_ok(a, mbw, planes, 1) && cm::conv_ups_ok(a, mbw, planes, 2) && cm::conv_ups_slots(a, mbw) <= MAX_SLOTS);
    a.C1 = 32;
    EXPECT(!cm::conv_ups_ok(a, mbw, planes, 1));           // concat sources / normalisation on load stay on the generic kernel
    a.C1 = 0; a.gn = reinterpret_cast<const float *>(&a);
    EXPECT(!cm::conv_ups_ok(a, mbw, planes, 1));
  }
  {
    int tz = 0, ty = 0, tx = 0, mbw = 0, planes = 0;
    EXPECT(cm::conv_ups_pick(4, 6, 18, &tz, &ty, &tx, &mbw, &planes) && tz == 4 && ty == 3 && tx == 9 && mbw == 4 && planes == 1);
    EXPECT(cm::conv_ups_pick(2, 3, 9, &tz, &ty, &tx, &mbw, &planes) && tz == 2 && ty == 3 && tx == 9 && mbw == 2 && planes == 1);
  }
  // the whole-sample kernel accepts the quarter resolution of the ATC / CR-120 grids and refuses what it cannot stage
  cm::QrArgs q{};
  q.C0 = 128; q.Co = 128; q.groups = 8; q.Y = 3; q.X = 9;
  EXPECT(cm::conv_qr_ok(q));
  q.Y = 7; q.X = 6; q.C1 = 128;
  EXPECT(cm::conv_qr_ok(q));
  q.Y = 6; q.X = 18;
  EXPECT(!cm::conv_qr_ok(q));                       // 108 voxels per plane
  q.Y = 3; q.X = 9; q.Co = 48;
  EXPECT(!cm::conv_qr_ok(q));
}

// conv_wino_form: the specialised launch forms of conv_wino_p_kernel are taken only for what they were compiled for; everything else
// -- a training launch (Dropout3d multiplier), more samples than sample lanes, a grid the full-resolution tile does not divide,
// diagnostic flags, another operand form -- gets the generic kernel (form 0)
void test_wino_form_dispatch() {
  const float dummy[4] = {0.f, 0.f, 0.f, 0.f};
  cm::ConvArgs full{};
  full.f16 = 4; full.silu = 1; full.gn = dummy; full.B = 64;
  full.C0 = 32; full.Co = 32; full.Zo = full.Zs = 8; full.Yo = full.Ys = 12; full.Xo = full.Xs = 36;
  full.bz = 8; full.by = 4; full.bx = 4; full.ntz = 1; full.nty = 3; full.ntx = 9;
  const int whole = cm::WINO_FORM_ONE | cm::WINO_FORM_PLAIN | cm::WINO_FORM_WHOLE;
  EXPECT(cm::conv_wino_form(full, 64) == whole);
  for (const int yx : {28 * 1000 + 24, 24 * 1000 + 72}) {            // CR-120 and the 2x grid divide by the tile as well
    cm::ConvArgs a = full;
    a.Yo = a.Ys = yx / 1000; a.Xo = a.Xs = yx % 1000; a.nty = a.Yo / 4; a.ntx = a.Xo / 4;
    EXPECT(cm::conv_wino_form(a, 64) == whole);
  }
  { cm::ConvArgs a = full; a.pm = dummy; EXPECT(cm::conv_wino_form(a, 64) == 0); }                 // training launch
  { cm::ConvArgs a = full; a.B = 96; EXPECT(cm::conv_wino_form(a, 64) == 0); }                     // B above the grid's sample lanes
  { cm::ConvArgs a = full; a.Yo = a.Ys = 10; a.Xo = a.Xs = 14; a.nty = 3; a.ntx = 4; EXPECT(cm::conv_wino_form(a, 64) == 0); }   // shifted last tiles
  { cm::ConvArgs a = full; a.dbg = 4096; EXPECT(cm::conv_wino_form(a, 64) == 0); }                 // diagnostic flags
  { cm::ConvArgs a = full; a.dbg = 1 << 20; EXPECT(cm::conv_wino_form(a, 64) == 0); }              // the documented force-generic bit
  { cm::ConvArgs a = full; a.f16 = 2; EXPECT(cm::conv_wino_form(a, 64) == 0); }                    // six-term form
  { cm::ConvArgs a = full; a.gn = nullptr; a.silu = 0; EXPECT(cm::conv_wino_form(a, 64) == 0); }   // raw source (no GroupNorm + SiLU)
  { cm::ConvArgs a = full; a.gp0 = dummy; EXPECT(cm::conv_wino_form(a, 64) == 0); }                // rows from two places
  { cm::ConvArgs a = full; a.Co = 48; EXPECT(cm::conv_wino_form(a, 64) == 0); }                    // partly filled channel tile
  cm::ConvArgs half{};
  half.f16 = 4; half.silu = 1; half.gn = dummy; half.B = 32;
  half.C0 = 64; half.Co = 64; half.Zo = half.Zs = 4; half.Yo = half.Ys = 6; half.Xo = half.Xs = 18;
  half.bz = 2; half.by = 6; half.bx = 10; half.ntz = 2; half.nty = 1; half.ntx = 2;
  EXPECT(cm::conv_wino_form(half, 32) == (cm::WINO_FORM_ONE | cm::WINO_FORM_PLAIN));
  { cm::ConvArgs a = half; a.gn = nullptr; a.gp0 = dummy; EXPECT(cm::conv_wino_form(a, 32) == (cm::WINO_FORM_ONE | cm::WINO_FORM_PLAIN | cm::WINO_FORM_OWNGN)); }
  { cm::ConvArgs a = half; a.B = 64; EXPECT(cm::conv_wino_form(a, 32) == 0); }
  { cm::ConvArgs a = half; a.pm = dummy; EXPECT(cm::conv_wino_form(a, 32) == 0); }
  { cm::ConvArgs a = half; a.dbg = 512; EXPECT(cm::conv_wino_form(a, 32) == 0); }
  { cm::ConvArgs a = half; a.Co = 32; EXPECT(cm::conv_wino_form(a, 32) == 0); }                    // one-tile workgroups: no h2 form at all
}

// conv_route: the one place that decides which kernel family and operand form a conv runs on.  Hand-built ops, one per layer class
// of the plan, carrying the fragment sets add_conv packs for each precision plan (dummy non-null pointers: the route only asks
// whether a set exists), crossed with precision x training forward x stale h2 x h2_off x debug steering.  Every combination is
// asserted against the table below (the kernel call tables under profiles/) AND against the invariants.
enum RouteClass { RC_WINO_FULL, RC_WINO_FULL_SKIP, RC_WINO_HALF, RC_WINO_HALF_SKIP, RC_QUARTER, RC_QUARTER_NO_TRAIN_QR, RC_KSPLIT, RC_STRIDE2,
                  RC_UPS_STATS, RC_UPS_NO_STATS, RC_FIRST, RC_LAST, RC_1X1, RC_1X1_STATS, RC_SKIP_ABSORBED, RC_COUNT };

Op route_class_op(int rc, int precision) {
  static float frag[4];
  static Act src, skip, out;
  const bool p32 = precision == CM_PRECISION_F32, p16 = precision == CM_PRECISION_F16;
  src.part = frag; skip.C = 64; out.C = 64;
  Op op;
  op.kind = OP_CONV; op.cls = K_CONV3;
  op.in0 = &src; op.out_act = &out;
  cm::ConvArgs &a = op.ca;
  a.ntaps = 27; a.td = 3; a.stride = 1; a.CK = 32; a.bs = a.bz = a.by = a.bx = 1; a.ntz = a.nty = a.ntx = 1;
  auto grid = [&](int Z, int Y, int X, int Ci, int Co) { a.Zs = a.Zo = Z; a.Ys = a.Yo = Y; a.Xs = a.Xo = X; a.C0 = Ci; a.Co = Co; a.out_cs = Co; };
  const bool skipc = rc == RC_WINO_FULL_SKIP || rc == RC_WINO_HALF_SKIP;
  switch (rc) {
    case RC_WINO_FULL: case RC_WINO_FULL_SKIP: case RC_WINO_HALF: case RC_WINO_HALF_SKIP: {
      const bool full = rc == RC_WINO_FULL || rc == RC_WINO_FULL_SKIP;
      if (full) grid(8, 12, 36, skipc ? 96 : 32, 32); else grid(4, 6, 18, skipc ? 192 : 64, 64);
      a.gn = frag; a.silu = 1; op.gn_op = 0; op.stat_act = &out; op.NB = 1;
      op.wino = true; op.d_wwino = frag;
      EXPECT(resolve_conv(nullptr, op) == 0 && op.wino && op.MB == 4);        // (a Winograd op that fits its tile touches no device)
      if (!p16) { EXPECT(cm::conv_wino_b6_ok(a.bz, a.by, a.bx, a.Co, a.Zo)); op.d_wwino_b6 = frag; }
      if (p32) op.d_wwino_h2 = frag;
      if (p16) {                                                              // (Z >= 4 on both grids: the direct f16 kernel)
        op.d_wwino16 = frag; op.f16d = true; op.d_w16d = frag;
        EXPECT(cm::conv_f16d_pick(a.Zo, a.Yo, a.Xo, &op.f16d_bz, &op.f16d_by, &op.f16d_bx, &op.f16d_mbw));
      }
      if (skipc) { op.d_s2w = op.d_bias_fused = frag; op.skip0 = &skip; op.pm_off = 0; if (p16) op.d_w16d_skip = frag; }
      break;
    }
    case RC_QUARTER: case RC_QUARTER_NO_TRAIN_QR:
      grid(2, 3, 9, 128, 128);
      a.gn = frag; a.silu = 1; op.gn_op = 0; op.stat_act = &out; op.NB = 2;
      op.ks = 4; op.d_zero_bias = frag;                                       // (the K-split set-up stays for the training forward)
      op.qr = true; op.d_wqr = frag;
      if (!p16) { op.d_wqr_b6 = frag; op.train_qr = rc == RC_QUARTER; }
      if (p32) op.d_wqr_h2 = frag;
      break;
    case RC_KSPLIT:    // stride-2 conv into the quarter resolution: statistics, no GroupNorm on load -> no whole-sample kernel
      grid(2, 3, 9, 64, 128); a.Zs = 4; a.Ys = 6; a.Xs = 18; a.stride = 2; op.stat_act = &out; op.NB = 2; op.ks = 2; op.d_zero_bias = frag;
      break;
    case RC_STRIDE2:
      grid(4, 6, 18, 32, 64); a.Zs = 8; a.Ys = 12; a.Xs = 36; a.stride = 2; op.stat_act = &out; op.NB = 2;
      break;
    case RC_UPS_STATS: case RC_UPS_NO_STATS:
      grid(8, 12, 36, 64, 64); a.Zs = 4; a.Ys = 6; a.Xs = 18; a.par = 1; a.ntaps = 8; a.td = 2; op.stat_act = &out; op.NB = 2;
      op.ups = true;
      EXPECT(cm::conv_ups_pick(a.Zs, a.Ys, a.Xs, &op.ups_tz, &op.ups_ty, &op.ups_tx, &op.ups_mbw, &op.ups_planes));
      if (!p16) op.d_wups_b6 = frag;
      if (p32) op.d_wups_h2 = frag;
      if (p16) { op.d_wups16 = frag; op.d_wfrag16 = frag; }
      break;
    case RC_FIRST:
      grid(8, 12, 36, 8, 32); a.CK = 8; op.stat_act = &out; op.first_k = true; op.d_wfirst = frag;
      break;
    case RC_LAST:
      grid(8, 12, 36, 32, 4); a.out_cs = 8; a.gn = frag; a.silu = 1; op.gn_op = 0;
      op.small_n = true; op.d_wsmall = frag;
      EXPECT(cm::conv_fin_pick(a.Yo, a.Xo, &op.fin_by, &op.fin_bx));
      op.fin = true; op.d_wfin = op.d_wfin_src = frag;
      if (p32) op.d_wfin_h2 = frag;
      if (p16) op.d_wfin16 = frag;
      break;
    case RC_1X1: case RC_1X1_STATS: case RC_SKIP_ABSORBED:
      grid(2, 3, 9, 128, 384); a.ntaps = 1; a.td = 1; a.CK = 128; op.cls = K_CONV1; op.NB = 2;
      if (rc == RC_1X1_STATS) op.stat_act = &out;
      else if (p16) op.d_w1x1_16 = frag;
      op.skip_if_fused = rc == RC_SKIP_ABSORBED;
      break;
  }
  return op;
}

void test_conv_route() {
  struct Want { ConvKernel kernel; ConvForm form; };
  // [class][plan]: inference forward of the F32 (default), F32X, F32R and F16 plans -- the F32X column is the default plan with
  // every H2 replaced by B6 (include/crowdmod_hip.h), the F32R one with B3 -- and [class][4 / 5]: the training forward of a
  // 32-bit plan (all three alike: six-term fragments, no h2, no relaxed form) and of the f16 plan (never an f16 operand).
  const ConvKernel QR = CONV_QR, KS = CONV_KSPLIT, UPS = CONV_UPS, F16D = CONV_F16D, WINO = CONV_WINO, FIRST = CONV_FIRST, FIN = CONV_FIN,
                   X11 = CONV_1X1_F16, GEN = CONV_GENERIC, NONE = CONV_NONE;
  const ConvForm FP32 = FORM_FP32, F16 = FORM_F16, B6 = FORM_B6, B3 = FORM_B3, H2 = FORM_H2;
  const Want want[RC_COUNT][6] = {
      /* WINO_FULL         */ {{WINO, H2}, {WINO, B6}, {WINO, B3}, {F16D, F16}, {WINO, B6}, {WINO, FP32}},
      /* WINO_FULL_SKIP    */ {{WINO, H2}, {WINO, B6}, {WINO, B3}, {F16D, F16}, {WINO, B6}, {WINO, FP32}},
      /* WINO_HALF         */ {{WINO, H2}, {WINO, B6}, {WINO, B3}, {F16D, F16}, {WINO, B6}, {WINO, FP32}},
      /* WINO_HALF_SKIP    */ {{WINO, H2}, {WINO, B6}, {WINO, B3}, {F16D, F16}, {WINO, B6}, {WINO, FP32}},
      /* QUARTER           */ {{QR, H2}, {QR, B6}, {QR, B3}, {QR, FP32}, {QR, B6}, {KS, FP32}},
      /* QUARTER_NO_TRAIN  */ {{QR, H2}, {QR, B6}, {QR, B3}, {QR, FP32}, {KS, FP32}, {KS, FP32}},
      /* KSPLIT            */ {{KS, FP32}, {KS, FP32}, {KS, FP32}, {KS, FP32}, {KS, FP32}, {KS, FP32}},
      /* STRIDE2           */ {{GEN, FP32}, {GEN, FP32}, {GEN, FP32}, {GEN, FP32}, {GEN, FP32}, {GEN, FP32}},
      /* UPS_STATS         */ {{UPS, H2}, {UPS, B6}, {UPS, B3}, {UPS, F16}, {UPS, B6}, {UPS, FP32}},
      /* UPS_NO_STATS      */ {{UPS, B6}, {UPS, B6}, {UPS, B3}, {UPS, F16}, {UPS, B6}, {UPS, FP32}},
      /* FIRST             */ {{FIRST, FP32}, {FIRST, FP32}, {FIRST, FP32}, {FIRST, FP32}, {FIRST, FP32}, {FIRST, FP32}},
      /* LAST              */ {{FIN, H2}, {FIN, B6}, {FIN, B3}, {FIN, F16}, {FIN, B6}, {FIN, B6}},
      /* 1X1               */ {{GEN, FP32}, {GEN, FP32}, {GEN, FP32}, {X11, F16}, {GEN, FP32}, {GEN, FP32}},
      /* 1X1_STATS         */ {{GEN, FP32}, {GEN, FP32}, {GEN, FP32}, {GEN, FP32}, {GEN, FP32}, {GEN, FP32}},
      /* SKIP_ABSORBED     */ {{NONE, FP32}, {NONE, FP32}, {NONE, FP32}, {NONE, FP32}, {GEN, FP32}, {GEN, FP32}},
  };
  const int plans[4] = {CM_PRECISION_F32, CM_PRECISION_F32X, CM_PRECISION_F32R, CM_PRECISION_F16};
  int walked = 0;
  for (int rc = 0; rc < RC_COUNT; ++rc)
    for (int pi = 0; pi < 4; ++pi)
      for (int train = 0; train < 2; ++train)
        for (int stale = 0; stale < 2; ++stale)
          for (int off = 0; off < 2; ++off)
            for (int dbg = 0; dbg < 3; ++dbg) {   // plain, dbg_raw, dbg_raw + dbg_h2
              Op op = route_class_op(rc, plans[pi]);
              op.h2_off = off; op.dbg_raw = dbg >= 1; op.dbg_h2 = dbg == 2;
              const bool src_stats = rc != RC_UPS_NO_STATS;            // does an earlier op of the forward write the source's slots?
              FwdCtx ctx;
              ctx.precision = plans[pi]; ctx.train_fwd = train; ctx.h2_stale = stale;
              OpPlan planned;
              EXPECT(plan_conv(op, ctx, src_stats ? 8 : 0, &planned).empty());
              const ConvRoute r = planned.route;
              ++walked;
              // the table: h2 where the default plan has it and nothing withdraws it, else what F32X runs
              const bool h2_live = !stale && !off && dbg != 1;
              const Want w = train ? want[rc][pi == 3 ? 5 : 4] : want[rc][(pi == 0 && !h2_live) ? 1 : pi];
              EXPECT(r.kernel == w.kernel && r.form == w.form);
              // the invariants
              if (r.form == FORM_H2) EXPECT(plans[pi] == CM_PRECISION_F32 && !train && !stale && !off && (!op.dbg_raw || op.dbg_h2) &&
                                            (op.d_wwino_h2 || op.d_wqr_h2 || op.d_wfin_h2 || (op.d_wups_h2 && src_stats)));
              if (train) EXPECT(r.form != FORM_F16 && r.form != FORM_B3 && r.kernel != CONV_F16D && r.kernel != CONV_1X1_F16 && r.kernel != CONV_NONE);
              if (train && r.kernel == CONV_QR) EXPECT(op.train_qr && op.d_wqr_b6);
              if (op.ks > 1) EXPECT(r.kernel == CONV_QR || r.kernel == CONV_KSPLIT);
              // the kernel FAMILY depends on the plan and on training / inference only: what plan_h16 decides
              // at finalize still holds when h2 goes stale, a bound is withdrawn or a debug hook steers the form
              EXPECT(r.kernel == conv_route(op, plans[pi], train, false).kernel);
              // f16 tensors: plan_h16 and the launch-time check ask route_takes_h16; it accepts what ConvArgs::h16 documents, no more
              for (int mask = 1; mask < 64; ++mask) {
                const bool takes = r.kernel == CONV_F16D || (r.kernel == CONV_UPS && r.form == FORM_F16 && !(mask & ~(1 | 4))) ||
                                   (r.kernel == CONV_FIRST && mask == 4) || ((r.kernel == CONV_FIN || r.kernel == CONV_SMALLN) && !(mask & ~(1 | 2)));
                EXPECT(route_takes_h16(r, mask) == takes);
              }
            }
  // the last conv off its matrix-core kernel: a Dropout3d multiplier (no such layer exists; the launcher refuses it) or a second source
  {
    Op op = route_class_op(RC_LAST, CM_PRECISION_F32);
    op.pm_off = 0;
    EXPECT(conv_route(op, CM_PRECISION_F32, true, false).kernel == CONV_SMALLN && conv_route(op, CM_PRECISION_F32, false, false).kernel == CONV_FIN);
    op.ca.C1 = 32;
    EXPECT(conv_route(op, CM_PRECISION_F32, false, false).kernel == CONV_SMALLN);
    walked += 3;
  }
  // a parity conv the stage-once kernel does not take: f16 fragments only where the generic launcher has an f16 instantiation
  {
    Op op = route_class_op(RC_UPS_STATS, CM_PRECISION_F16);
    op.d_wups16 = nullptr;
    op.MB = 5; op.NB = 1; op.ca.bz = 4; op.ca.by = 6; op.ca.bx = 6;
    ConvRoute r = conv_route(op, CM_PRECISION_F16, false, false);
    EXPECT(r.kernel == CONV_GENERIC && r.form == FORM_F16);
    op.ca.bx = 5;
    r = conv_route(op, CM_PRECISION_F16, false, false);
    EXPECT(r.kernel == CONV_GENERIC && r.form == FORM_FP32);
    r = conv_route(op, CM_PRECISION_F16, true, false);
    EXPECT(r.kernel == CONV_UPS && r.form == FORM_FP32);
    walked += 3;
  }
  printf("test_conv_route: %d combinations walked\n", walked);
}

// plan_forward: everything a forward's launches depend on -- which ops run, each conv's route, the slot count of every statistics
// tensor, who finalises each GroupNorm -- decided in one pure walk.  Hand-built op lists (route_class_op wired through Act objects
// and OP_GNFIN ops) are asserted against written-out tables for the four precision plans x inference / training, and every plan
// against the invariants of check_plan.
struct PlanList {
  std::vector<std::unique_ptr<Act>> acts;   // (the ops point into them)
  std::vector<Op> ops;
  Act *act(int C, int Z, int Y, int X) {
    static float buf[4];
    acts.push_back(std::make_unique<Act>());
    Act *a = acts.back().get();
    a->C = C; a->Z = Z; a->Y = Y; a->X = X; a->part = a->cnt = buf;
    return a;
  }
  // a conv of class `rc`: sources in0 (+ in1), output `out` (its statistics too when the class writes them), normalised by op `gn`
  int conv(int rc, int precision, const Act *in0, Act *out, int gn = -1, const Act *in1 = nullptr) {
    Op op = route_class_op(rc, precision);
    op.in0 = in0; op.in1 = in1; op.out_act = out;
    if (op.stat_act) op.stat_act = out;
    op.gn_op = gn;
    if (gn < 0) op.ca.gn = nullptr;
    else if (op.qr) ops[gn].qr_consumer = true;               // (add_conv)
    op.label = "conv" + std::to_string(ops.size());
    ops.push_back(op);
    return (int)ops.size() - 1;
  }
  int gnfin(const Act *g0, const Act *g1 = nullptr) {
    Op op;
    op.kind = OP_GNFIN; op.cls = K_NORM; op.g0 = g0; op.g1 = g1; op.label = "gn" + std::to_string(ops.size());
    ops.push_back(op);
    return (int)ops.size() - 1;
  }
};

bool operator==(const OpPlan &a, const OpPlan &b) {
  return a.launch == b.launch && a.route.kernel == b.route.kernel && a.route.form == b.route.form && a.ns_out == b.ns_out && a.ns0 == b.ns0 &&
         a.ns1 == b.ns1 && a.fin == b.fin && a.carries == b.carries;
}

FwdCtx plan_ctx(int precision, bool train, bool stale = false, int B = 2) {
  FwdCtx c;
  c.precision = precision; c.train_fwd = train; c.h2_stale = stale; c.B = B;
  return c;
}

// the invariants of every plan
void check_plan(const std::vector<Op> &ops, const FwdCtx &ctx) {
  const FwdPlan P = plan_forward(ops, ctx);
  EXPECT(P.err.empty() && P.ops.size() == ops.size());
  EXPECT(plan_forward(ops, ctx).ops == P.ops);                 // planning twice gives equal plans
  const int n = (int)ops.size();
  std::map<const Act *, int> written;                          // by the launched ops so far
  for (int i = 0; i < n; ++i) {
    const Op &op = ops[i];
    const OpPlan &p = P.ops[i];
    const bool in_ctx = op.kind == OP_ATTNBLK ? !ctx.train_fwd : !(op.in_attn_block && !ctx.train_fwd);
    if (!in_ctx) { EXPECT(!p.launch && p.fin == FIN_NONE && p.carries < 0 && p.ns_out == 0); continue; }
    if (op.kind == OP_CONV) {
      EXPECT(p.route.kernel == conv_route(op, ctx.precision, ctx.train_fwd, ctx.h2_stale).kernel);   // the family: conv_route's, always
      EXPECT(p.launch == (p.route.kernel != CONV_NONE));
      if (p.route.kernel == CONV_UPS && p.route.form == FORM_H2) EXPECT(p.ns0 >= 1 && written.count(op.in0) && written[op.in0] == p.ns0);
    }
    if (p.carries >= 0) {
      EXPECT(p.launch && p.carries > i && ops[p.carries].kind == OP_GNFIN && P.ops[p.carries].fin == FIN_COMBINE);
      EXPECT(op.kind == OP_ATTNBLK || p.route.kernel == CONV_KSPLIT);
    }
    if (p.ns_out) {
      EXPECT(p.launch && p.ns_out >= 1 && p.ns_out <= MAX_SLOTS);
      written[op.kind == OP_CONV ? op.stat_act : op.kind == OP_ATTNBLK ? op.ab_out : op.act] = p.ns_out;
    }
    if (op.kind != OP_GNFIN) { EXPECT(p.fin == FIN_NONE); continue; }
    // exactly one disposition, and its counterpart agrees
    EXPECT(p.fin != FIN_NONE && p.launch == (p.fin == FIN_ALONE));
    int carriers = 0, cons = -1, ncons = 0;
    for (int j = 0; j < n; ++j) {
      if (P.ops[j].carries == i) ++carriers;
      if (ops[j].kind == OP_CONV && ops[j].gn_op == i && P.ops[j].launch) { if (cons < 0) cons = j; ++ncons; }
    }
    EXPECT(carriers == (p.fin == FIN_COMBINE ? 1 : 0));
    // a finalisation left to a consumer has exactly one launched consumer, and that launch does take the slots
    if (p.fin == FIN_QR || p.fin == FIN_WINO) EXPECT(ncons == 1);
    if (p.fin == FIN_WINO) EXPECT(cons > i && wino_merges(ops[cons], P.ops[cons].route, ctx.B));
    if (p.fin == FIN_QR) EXPECT(!ctx.train_fwd && op.qr_consumer && cons > i && P.ops[cons].route.kernel == CONV_QR);
    if (p.fin == FIN_WINO) EXPECT(!ctx.train_fwd && cons > i && P.ops[cons].route.form != FORM_FP32 && P.ops[cons].route.kernel == CONV_WINO && p.ns0 <= 16 && p.ns1 <= 16 &&
                                  (!op.g1 || op.g1->V() == op.g0->V()));
    if (op.qr_consumer && !ctx.train_fwd) EXPECT(p.fin == FIN_QR);
    // every slot count a consumer reads was assigned by an earlier launched op
    EXPECT(written.count(op.g0) && p.ns0 == written[op.g0] && p.ns0 >= 1 && p.ns0 <= MAX_SLOTS);
    if (op.g1) EXPECT(written.count(op.g1) && p.ns1 == written[op.g1] && p.ns1 >= 1 && p.ns1 <= MAX_SLOTS);
  }
}

void test_forward_plan() {
  const int plans[4] = {CM_PRECISION_F32, CM_PRECISION_F32X, CM_PRECISION_F32R, CM_PRECISION_F16};
  const ConvForm infer_form[4] = {FORM_H2, FORM_B6, FORM_B3, FORM_FP32};   // of the whole-sample quarter-resolution conv
  int walked = 0;
  for (int pi = 0; pi < 4; ++pi) {
    const int prec = plans[pi];
    const bool p16 = prec == CM_PRECISION_F16;
    // ---- K-split conv -> GNFIN -> quarter-resolution conv -> GNFIN -> quarter-resolution conv -------------------------------------
    // at 2 x 3 x 9 (54 voxels: two slots from either kernel) and at 2 x 6 x 6 (72 voxels: three slots from a K-split combine, four
    // from conv_qr2, and too many voxels for a combine to carry a finalisation)
    for (int tq = 0; tq < 2; ++tq)
      for (int big = 0; big < 2; ++big) {
        PlanList L;
        const int Y = big ? 6 : 3, X = big ? 6 : 9, ks_ns = big ? 3 : 2, qr_ns = big ? 4 : 2;
        Act *s = L.act(64, 4, 2 * Y, 2 * X), *a = L.act(128, 2, Y, X), *b = L.act(128, 2, Y, X), *c = L.act(128, 2, Y, X);
        const int qclass = tq ? RC_QUARTER : RC_QUARTER_NO_TRAIN_QR;
        L.conv(RC_KSPLIT, prec, s, a);                 // 0
        L.gnfin(a);                                    // 1
        L.conv(qclass, prec, a, b, 1);                 // 2
        L.gnfin(b);                                    // 3
        L.conv(qclass, prec, b, c, 3);                 // 4
        for (int i : {0, 2, 4}) {
          cm::ConvArgs &g = L.ops[i].ca;
          g.Yo = Y; g.Xo = X; g.Ys = (i ? 1 : 2) * Y; g.Xs = (i ? 1 : 2) * X;
        }
        for (int stale = 0; stale < 2; ++stale) {
          const FwdCtx ctx = plan_ctx(prec, false, stale);
          check_plan(L.ops, ctx);
          const FwdPlan P = plan_forward(L.ops, ctx);
          // inference: both finalisations belong to their conv_qr2 consumers, the combine carries nothing
          EXPECT(P.ops[0].route.kernel == CONV_KSPLIT && P.ops[0].ns_out == ks_ns && P.ops[0].carries == -1);
          EXPECT(P.ops[1].fin == FIN_QR && !P.ops[1].launch && P.ops[1].ns0 == ks_ns);
          EXPECT(P.ops[2].route.kernel == CONV_QR && P.ops[2].ns_out == qr_ns);
          if (!big) EXPECT(P.ops[2].route.form == ((pi == 0 && stale) ? FORM_B6 : infer_form[pi]));
          EXPECT(P.ops[3].fin == FIN_QR && P.ops[3].ns0 == qr_ns && P.ops[4].route.kernel == CONV_QR && P.ops[4].carries == -1);
          ++walked;
        }
        const FwdCtx ctx = plan_ctx(prec, true);
        check_plan(L.ops, ctx);
        const FwdPlan P = plan_forward(L.ops, ctx);
        // training: the K-split conv's combine carries the finalisation (the backward needs its mean / rstd rows) where the geometry
        // allows; with train_qr (32-bit plans) the consumer is conv_qr2, a one-pass kernel, so the next finalisation launches alone;
        // without, the consumer is the K-split kernel -- with ITS slot count, not the inference plan's -- and its combine carries the next
        const bool qr_trains = tq && !p16;
        EXPECT(P.ops[0].route.kernel == CONV_KSPLIT && P.ops[0].ns_out == ks_ns && P.ops[0].carries == (big ? -1 : 1));
        EXPECT(P.ops[1].fin == (big ? FIN_ALONE : FIN_COMBINE) && P.ops[1].launch == (big != 0) && P.ops[1].ns0 == ks_ns);
        EXPECT(P.ops[2].route.kernel == (qr_trains ? CONV_QR : CONV_KSPLIT) && P.ops[2].ns_out == (qr_trains ? qr_ns : ks_ns));
        if (!big) EXPECT(P.ops[2].route.form == (qr_trains ? FORM_B6 : FORM_FP32));
        const bool carried = !qr_trains && !big;
        EXPECT(P.ops[2].carries == (carried ? 3 : -1) && P.ops[3].fin == (carried ? FIN_COMBINE : FIN_ALONE) && P.ops[3].launch == !carried &&
               P.ops[3].ns0 == P.ops[2].ns_out);
        ++walked;
      }
    // ---- stride-2 generic conv -> GNFIN -> half-resolution Winograd conv: 16 slots, 18 slots ----------------------
    for (int many = 0; many < 2; ++many)
      for (int w16 = 0; w16 < 2; ++w16) {            // w16: under the f16 plan, the consumer outside the direct f16 kernel (Winograd on f16 fragments)
        PlanList L;
        Act *s = L.act(32, 8, 12, 36), *h = L.act(64, 4, 6, 18), *o = L.act(64, 4, 6, 18);
        L.conv(RC_STRIDE2, prec, s, h);              // 0
        L.gnfin(h);                                  // 1
        L.conv(RC_WINO_HALF, prec, h, o, 1);         // 2
        Op &prod = L.ops[0];
        prod.ca.ntz = 2; prod.ca.nty = 1; prod.ca.ntx = many ? 3 : 2; prod.MB = many ? 3 : 4;      // 16 or 18 slots
        if (w16) L.ops[2].f16d = false;
        const bool wino = !p16 || w16;               // the consumer's inference route is the Winograd kernel on split or f16 fragments
        for (const int B : {2, 64}) {
          const FwdCtx ctx = plan_ctx(prec, false, false, B);
          check_plan(L.ops, ctx);
          const FwdPlan P = plan_forward(L.ops, ctx);
          EXPECT(P.ops[0].route.kernel == CONV_GENERIC && P.ops[0].ns_out == (many ? 18 : 16) && P.ops[1].ns0 == P.ops[0].ns_out);
          EXPECT(P.ops[2].route.kernel == (wino ? CONV_WINO : CONV_F16D));
          // f16 fragments: the persistent kernel only when the two-tile grid fills the chip (4 tiles x 64 samples = 256 workgroups)
          const bool merged = !many && wino && (!p16 || B == 64);
          EXPECT(P.ops[1].fin == (merged ? FIN_WINO : FIN_ALONE) && P.ops[1].launch == !merged);
          if (wino) EXPECT(P.ops[2].ns_out == 2 * 1 * 2 * 4);   // 2 x 6 x 10 tiles on 4 x 6 x 18, four sub-blocks each
          ++walked;
        }
        const FwdCtx ctx = plan_ctx(prec, true);
        check_plan(L.ops, ctx);
        const FwdPlan P = plan_forward(L.ops, ctx);
        EXPECT(P.ops[1].fin == FIN_ALONE && P.ops[1].launch && P.ops[2].route.kernel == CONV_WINO && P.ops[2].route.form == (p16 ? FORM_FP32 : FORM_B6));
        ++walked;
      }
    // ---- Winograd conv with statistics -> upsample conv --------------------------------------------------------------------------
    {
      PlanList L;
      Act *s = L.act(64, 4, 6, 18), *h = L.act(64, 4, 6, 18), *u = L.act(64, 8, 12, 36);
      L.conv(RC_WINO_HALF, prec, s, h);              // 0
      L.conv(RC_UPS_STATS, prec, h, u);              // 1
      const ConvForm six[4] = {FORM_B6, FORM_B6, FORM_B3, FORM_F16};
      for (int stale = 0; stale < 2; ++stale) {
        const FwdCtx ctx = plan_ctx(prec, false, stale);
        check_plan(L.ops, ctx);
        const FwdPlan P = plan_forward(L.ops, ctx);
        EXPECT(P.ops[0].route.kernel == (p16 ? CONV_F16D : CONV_WINO) && P.ops[0].ns_out >= 1 && P.ops[1].ns0 == P.ops[0].ns_out);
        EXPECT(P.ops[1].route.kernel == CONV_UPS && P.ops[1].route.form == ((pi == 0 && !stale) ? FORM_H2 : six[pi]));   // h2 on the default plan
        ++walked;
      }
      check_plan(L.ops, plan_ctx(prec, true));
      // no earlier op writes the source's slots: the six-term form
      std::vector<Op> alone(L.ops.begin() + 1, L.ops.end());
      check_plan(alone, plan_ctx(prec, false));
      const FwdPlan P = plan_forward(alone, plan_ctx(prec, false));
      EXPECT(P.ops[0].route.kernel == CONV_UPS && P.ops[0].route.form == six[pi] && P.ops[0].ns0 == 0);
      ++walked;
    }
    // ---- K-split conv -> attention block (four generic ops + the fused one) -> GNFIN -> 1x1x1 conv ----------------------------------
    {
      PlanList L;
      Act *s = L.act(64, 4, 6, 18), *x = L.act(128, 2, 3, 9), *qkv = L.act(384, 2, 3, 9), *core = L.act(128, 2, 3, 9), *o = L.act(128, 2, 3, 9),
          *y = L.act(384, 2, 3, 9);
      L.conv(RC_KSPLIT, prec, s, x);                 // 0
      L.gnfin(x);                                    // 1  attention.group_norm
      L.conv(RC_1X1, prec, x, qkv, 1);               // 2
      { Op at; at.kind = OP_ATTN; at.cls = K_ATTN; at.S = 54; at.E = 128; L.ops.push_back(at); }   // 3
      L.conv(RC_1X1_STATS, prec, core, o);           // 4  out_proj (+ residual), statistics
      for (int i = 1; i <= 4; ++i) L.ops[i].in_attn_block = true;
      { Op fb; fb.kind = OP_ATTNBLK; fb.cls = K_ATTN; fb.ab_x = x; fb.ab_out = o; fb.S = 54; fb.E = 128; fb.ab_gn = 1; fb.ab_qkv = 2; fb.ab_outc = 4; L.ops.push_back(fb); }   // 5
      L.gnfin(o);                                    // 6
      L.conv(RC_1X1, prec, o, y, 6);                 // 7
      check_plan(L.ops, plan_ctx(prec, false));
      FwdPlan P = plan_forward(L.ops, plan_ctx(prec, false));
      // inference: the fused block; its head-sum combine carries the next finalisation; the K-split conv in front of it carries nothing
      // (the block normalises its input itself)
      for (int i = 1; i <= 4; ++i) EXPECT(!P.ops[i].launch);
      EXPECT(P.ops[0].carries == -1 && P.ops[5].launch && P.ops[5].ns_out == 2 && P.ops[5].carries == 6 && P.ops[6].fin == FIN_COMBINE && P.ops[6].ns0 == 2);
      check_plan(L.ops, plan_ctx(prec, true));
      P = plan_forward(L.ops, plan_ctx(prec, true));
      // training: the four generic ops instead; the K-split conv's combine carries the block's own GroupNorm
      EXPECT(!P.ops[5].launch && P.ops[0].carries == 1 && P.ops[1].fin == FIN_COMBINE && P.ops[2].launch && P.ops[3].launch && P.ops[4].launch);
      EXPECT(P.ops[4].ns_out == 1 && P.ops[6].fin == FIN_ALONE && P.ops[6].launch && P.ops[6].ns0 == 1);
      walked += 2;
    }
    // ---- a concat finalisation whose two sources disagree on the voxel count: never carried, never merged ---------------------------
    {
      PlanList L;
      Act *s = L.act(32, 8, 12, 36), *h = L.act(64, 4, 6, 18), *a = L.act(128, 2, 3, 9), *o = L.act(64, 4, 6, 18);
      L.conv(RC_STRIDE2, prec, s, h);                // 0
      L.conv(RC_KSPLIT, prec, h, a);                 // 1
      L.gnfin(a, h);                                 // 2
      L.conv(RC_WINO_HALF_SKIP, prec, a, o, 2, h);   // 3
      for (int train = 0; train < 2; ++train) {
        check_plan(L.ops, plan_ctx(prec, train));
        const FwdPlan P = plan_forward(L.ops, plan_ctx(prec, train));
        EXPECT(P.ops[1].carries == -1 && P.ops[2].fin == FIN_ALONE && P.ops[2].launch && P.ops[2].ns0 == 2 && P.ops[2].ns1 == 1);
        // the stand-alone launch path reports the existing error (before it launches anything)
        EXPECT(run_gnfin(L.ops[2], P.ops[2], 2, nullptr, 0) != 0 && std::string(cm_last_error()) == "concat sources disagree on voxel count");
        ++walked;
      }
      // the same list with equal voxel counts is carried
      L.acts[1]->Z = 2; L.acts[1]->Y = 3; L.acts[1]->X = 9;
      check_plan(L.ops, plan_ctx(prec, false));
      EXPECT(plan_forward(L.ops, plan_ctx(prec, false)).ops[2].fin == FIN_COMBINE);
      ++walked;
    }
  }
  // a statistics tensor nobody writes, and a slot count beyond the buffers: errors of the plan, not of a launch
  {
    PlanList L;
    Act *a = L.act(128, 2, 3, 9), *b = L.act(128, 2, 3, 9);
    L.gnfin(a);
    L.conv(RC_WINO_HALF, CM_PRECISION_F32, a, b, 0);
    EXPECT(!plan_forward(L.ops, plan_ctx(CM_PRECISION_F32, false)).err.empty());
    PlanList M;
    Act *s = M.act(32, 8, 12, 36), *h = M.act(64, 4, 6, 18);
    M.conv(RC_STRIDE2, CM_PRECISION_F32, s, h);
    M.ops[0].ca.ntz = 4; M.ops[0].ca.nty = 6; M.ops[0].ca.ntx = 6; M.ops[0].MB = 4;               // 576 slots
    EXPECT(!plan_forward(M.ops, plan_ctx(CM_PRECISION_F32, false)).err.empty());
    M.ops[0].ca.ntz = 2;                                                                            // 288
    EXPECT(plan_forward(M.ops, plan_ctx(CM_PRECISION_F32, false)).err.empty());
    walked += 3;
  }
  printf("test_forward_plan: %d plans checked\n", walked);
}

// The sampling loop's launch ranges of the UNet's two end convs (loop_ends_plan, conv_first_const_ztiles, conv_fin_zloop)
void test_loop_ends() {
  // first conv: pick_tile_first's tile on the three benchmark grids and the odd ones; with P = 5 every bz divides P - 1 = 4
  struct G { int Y, X, bz, by; };
  const G grids[] = {{12, 36, 4, 3}, {28, 24, 4, 4}, {24, 72, 2, 3}, {13, 37, 1, 13}, {11, 35, 1, 11}};
  for (const G &g : grids) {
    Op op = route_class_op(RC_FIRST, CM_PRECISION_F32);
    op.ca.Zo = op.ca.Zs = 8; op.ca.Yo = op.ca.Ys = g.Y; op.ca.Xo = op.ca.Xs = g.X;
    pick_tile_first(op);
    EXPECT(op.ca.bz == g.bz && op.ca.by == g.by && op.ca.ntz == 8 / g.bz);
    const int t = cm::conv_first_const_ztiles(op.ca.bz, op.ca.ntz, 5);
    EXPECT(t == 4 / g.bz && 2 * t == op.ca.ntz);              // exactly half of the z tiles are constant
    for (int tz = 0; tz < op.ca.ntz; ++tz) EXPECT((tz < t) == (tz * g.bz + g.bz <= 4));   // launched <=> the tile reaches plane P - 1 or above
  }
  // P / F combinations: the skipped tiles never reach the last past frame's output plane; no constant tile => the full launch
  for (int P = 1; P <= 9; ++P)
    for (int F = 1; F <= 4; ++F)
      for (int bz = 1; bz <= P + F; ++bz) {
        if ((P + F) % bz) continue;
        const int ntz = (P + F) / bz, t = cm::conv_first_const_ztiles(bz, ntz, P);
        EXPECT(t >= 0 && t < ntz && t * bz <= P - 1);
        EXPECT(((P - 1) % bz == 0 && P > 1) ? t == (P - 1) / bz : t == 0);
      }
  EXPECT(cm::conv_first_const_ztiles(4, 2, 1) == 0 && cm::conv_first_const_ztiles(1, 2, 1) == 0 && cm::conv_first_const_ztiles(3, 3, 5) == 0);
  // last conv: input planes of an output plane range; every kept output still meets its taps in the order dz = 0, 1, 2
  for (int P = 1; P <= 6; ++P)
    for (int F = 1; F <= 4; ++F) {
      const int Z = P + F;
      int zs, zl;
      cm::conv_fin_zloop(P, Z, Z, &zs, &zl);
      EXPECT(zs == P - 1 && zl == Z);
      cm::conv_fin_zloop(0, Z, Z, &zs, &zl);
      EXPECT(zs == 0 && zl == Z);                              // the whole range: the loop of a stand-alone forward
      cm::conv_fin_zloop(0, 1, Z, &zs, &zl);
      EXPECT(zs == 0 && zl == 2);
    }
  // the plan: both ends on their kernels, each switch alone, a last conv off the matrix-core kernel, other frame counts
  {
    static float x8, eps;
    std::vector<Op> ops;
    ops.push_back(route_class_op(RC_FIRST, CM_PRECISION_F32));
    ops.push_back(route_class_op(RC_WINO_FULL, CM_PRECISION_F32));
    ops.push_back(route_class_op(RC_LAST, CM_PRECISION_F32));
    ops[0].ca.src0 = &x8; pick_tile_first(ops[0]);
    ops[2].ca.out = &eps;
    LoopEnds le = loop_ends_plan(ops, &x8, &eps, 7, CM_PRECISION_F32, false, 5, 3, 4, 4);
    EXPECT(le.tz_first == 1 && le.zo_first == 5 && le.zo_end == 8 && le.fuse == 1);
    le = loop_ends_plan(ops, &x8, &eps, 15, CM_PRECISION_F32, false, 5, 3, 4, 4);
    EXPECT(le.fuse == 2);
    le = loop_ends_plan(ops, &x8, &eps, 0, CM_PRECISION_F32, false, 5, 3, 4, 4);
    EXPECT(le.tz_first == 0 && le.zo_end == 0 && le.fuse == 0);
    le = loop_ends_plan(ops, &x8, &eps, 1, CM_PRECISION_F32, false, 5, 3, 4, 4);
    EXPECT(le.tz_first == 0 && le.zo_first == 5 && le.zo_end == 8 && le.fuse == 0);
    le = loop_ends_plan(ops, &x8, &eps, 4, CM_PRECISION_F32, false, 5, 3, 4, 4);
    EXPECT(le.tz_first == 1 && le.zo_end == 0 && le.fuse == 0);
    le = loop_ends_plan(ops, &x8, &eps, 7, CM_PRECISION_F32, false, 1, 7, 4, 4);     // P = 1: no constant tile
    EXPECT(le.tz_first == 0 && le.zo_first == 1 && le.zo_end == 8 && le.fuse == 1);
    le = loop_ends_plan(ops, &x8, &eps, 7, CM_PRECISION_F32, false, 7, 1, 4, 4);     // F = 1; bz = 4 does not divide 6
    EXPECT(le.tz_first == 0 && le.zo_first == 7 && le.zo_end == 8 && le.fuse == 1);
    le = loop_ends_plan(ops, &x8, &eps, 7, CM_PRECISION_F32, false, 5, 3, 3, 4);     // channel counts differ: the separate sampler launch
    EXPECT(le.zo_end == 8 && le.fuse == 0);
    ops[2].ca.C1 = 32;                                                                // last conv on conv_smalln: all planes, separate launch
    le = loop_ends_plan(ops, &x8, &eps, 7, CM_PRECISION_F32, false, 5, 3, 4, 4);
    EXPECT(le.tz_first == 1 && le.zo_end == 0 && le.fuse == 0);
    ops[0].first_k = false;                                                           // first conv on the generic kernel
    le = loop_ends_plan(ops, &x8, &eps, 7, CM_PRECISION_F32, false, 5, 3, 4, 4);
    EXPECT(le.tz_first == 0);
  }
  // the fused update's launch predicate: the conv and the step must describe the same tensors
  {
    Op op = route_class_op(RC_LAST, CM_PRECISION_F32);
    cm::ConvArgs a = op.ca;
    a.by = op.fin_by; a.bx = op.fin_bx; a.B = 2; a.zo_first = 5; a.zo_end = 8;
    static float x;
    cm::StepArgs st{};
    st.x = &x; st.B = 2; st.C = 4; st.H = 12; st.W = 36; st.P = 5; st.F = 3; st.cs = 8;
    EXPECT(cm::conv_fin_fuse_ok(a, st));
    st.F = 2; EXPECT(!cm::conv_fin_fuse_ok(a, st)); st.F = 3;
    st.C = 3; EXPECT(!cm::conv_fin_fuse_ok(a, st)); st.C = 4;
    a.zo_first = 4; EXPECT(!cm::conv_fin_fuse_ok(a, st)); a.zo_first = 5;
    st.B = 1; EXPECT(!cm::conv_fin_fuse_ok(a, st));
  }
  printf("test_loop_ends ok\n");
}

void test_misc_errors() {
  EXPECT(cm_abi_version() == CM_ABI_VERSION);
  EXPECT(cm_device_count(nullptr) != 0);
  EXPECT(cm_model_destroy(nullptr) == 0);
  EXPECT(cm_schedule_destroy(nullptr) == 0);
  EXPECT(cm_train_set_lr(nullptr, 1.f) != 0);
  EXPECT(cm_train_set_sample_base(nullptr, 0) != 0);
  int32_t n = 0;
  EXPECT(cm_model_num_params(nullptr, &n) != 0);
  EXPECT(cm_profile_enable(nullptr, 1) != 0);
  EXPECT(cm_frame_metrics(0, nullptr, nullptr, 1, 1, 1, 1, 1, nullptr, nullptr) != 0);
  EXPECT(std::string(cm_last_error()).size() > 0);
  // the SSIM / energy / motion-feature entry points refuse before any device call (the pointers are never dereferenced)
  {
    const float *d = reinterpret_cast<const float *>(0x1000);
    double r[3] = {1, 1, 1}, o[8];
    EXPECT(cm_ssim_frames(0, nullptr, d, 1, 3, 8, 8, 1, r, o) != 0);
    EXPECT(cm_ssim_frames(0, d, d, 1, 3, 6, 8, 1, r, o) != 0 && std::string(cm_last_error()).find("6 x 8") != std::string::npos);
    EXPECT(cm_ssim_frames(0, d, d, 1, 3, 8, 129, 8, r, o) != 0 && std::string(cm_last_error()).find("W * F = 1032") != std::string::npos);
    EXPECT(cm_energy(0, d, 1, 2, 8, 8, 2, 1.f, 1.f, nullptr, o) != 0 && std::string(cm_last_error()).find("C = 2") != std::string::npos);
    EXPECT(cm_energy(0, d, 1, 3, 8, 8, 0, 1.f, 1.f, nullptr, o) != 0 && std::string(cm_last_error()).find("L = 0") != std::string::npos);
    EXPECT(cm_motion_feature_vectors(0, d, 1, 3, 8, 8, 2, 0, 4, 0.5, o, o) != 0 && std::string(cm_last_error()).find("f = 0") != std::string::npos);
    EXPECT(cm_motion_feature_tables(0, d, d, 1, 3, 8, 8, 2, 1, -1, 0.5, o) != 0 && std::string(cm_last_error()).find("k = -1") != std::string::npos);
    EXPECT(cm_motion_feature_tables(0, d, d, 1, 3, 8, 8, 2, 1, 4, 0.5, nullptr) != 0);
    EXPECT(cm::motion_feature_volumes(12, 36, 3, 1, 4) == 81 && cm::motion_feature_volumes(12, 36, 3, 2, 5) == 48);
    EXPECT(cm::ssim_frames_ok(128, 8) && !cm::ssim_frames_ok(147, 7));
  }
  // linspace restatement: endpoints and symmetry
  EXPECT(linspace_f32(0.f, 1.f, 10, 0) == 0.f && linspace_f32(0.f, 1.f, 10, 9) == 1.f && linspace_f32(3.f, 5.f, 1, 0) == 3.f);
}

// The optimizer store's layout (cm_opt_store.inc): offsets are the prefix sums of the tensor sizes, the trainable ranges the
// complement of the frozen tensors, never an empty one; and the store's refusals that need no device.
void test_opt_store() {
  using Ranges = std::vector<std::pair<size_t, size_t>>;
  auto params = [](std::vector<std::vector<int64_t>> shapes) {
    std::vector<Param> ps;
    for (auto &s : shapes) { Param p; p.name = "t" + std::to_string(ps.size()); p.shape = s; ps.push_back(p); }
    return ps;
  };
  for (const auto &ps : {params({{5}, {3, 2}, {7}, {2, 1, 2}}), params({{1000, 16}, {16, 3, 3, 3}, {16}, {1}, {9}}), params({{3}, {1}, {4}, {1}})}) {
    std::vector<size_t> off;
    size_t n = 0;
    for (const Param &p : ps) { off.push_back(n); n += (size_t)p.numel(); }
    const int last = (int)ps.size() - 1;
    const OptLayout a = opt_layout(ps, {0}), b = opt_layout(ps, {2}), c = opt_layout(ps, {});
    EXPECT(a.off == off && b.off == off && c.off == off && a.nfloats == n && b.nfloats == n && c.nfloats == n);
    EXPECT((a.ranges == Ranges{{off[1], n}} && b.ranges == Ranges{{0, off[2]}, {off[3], n}} && c.ranges == Ranges{{0, n}}));
    EXPECT((opt_layout(ps, {last}).ranges == Ranges{{0, off[last]}}));            // a frozen last tensor: no empty tail
    EXPECT((opt_layout(ps, {1, 2}).ranges == Ranges{{0, off[1]}, {off[3], n}}));  // adjacent frozen tensors: nothing between them
    OptStore S;
    static_cast<OptLayout &>(S) = b;
    size_t o = ~(size_t)0;
    EXPECT(S.find(ps, "t2", ps[2].numel(), &o) == 0 && o == off[2]);
    EXPECT(S.find(ps, "t9", 1, &o) != 0 && strstr(cm_last_error(), "unknown parameter t9"));
    EXPECT(S.find(ps, "t2", ps[2].numel() + 1, &o) != 0 && strstr(cm_last_error(), "size mismatch for t2") && o == off[2]);
    int32_t s = 4, neg = -1;
    EXPECT(S.opt_step(&s, 1) == 0 && s == 4 && S.step == 4);
    EXPECT(S.opt_step(&neg, 1) != 0 && strstr(cm_last_error(), "must be >= 0") && S.step == 4 && neg == -1);
    EXPECT(S.opt_step(&neg, 0) == 0 && neg == 4 && S.opt_step(nullptr, 0) != 0);
  }
  // the UNet family's accessors take which 0 and 1 only, and say so before they look at the handle
  float x = 0.f;
  for (int which : {-1, 2, 3}) {
    EXPECT(cm_train_get_opt_state(nullptr, "first.bias", which, &x, 1) != 0 && strstr(cm_last_error(), "0 = exp_avg, 1 = exp_avg_sq"));
    EXPECT(cm_train_set_opt_state(nullptr, "first.bias", which, &x, 1) != 0 && strstr(cm_last_error(), "0 = exp_avg, 1 = exp_avg_sq"));
  }
  EXPECT(cm_train_get_opt_state(nullptr, "first.bias", 1, &x, 1) != 0 && strstr(cm_last_error(), "bad argument"));
  printf("test_opt_store ok\n");
}

// wgrad_route / dgrad_route: the one place that decides which kernel a conv's weight gradient and data gradient run on.  The fifteen
// layer classes of test_conv_route (with the backward's facts added: reference taps, an output tensor of the op's own width, the
// UNet input as the first conv's source), crossed with precision x autocast x f16 fragments x every kernel-disabling switch, against
// the table below -- written from cm_train_host.inc as it stood before the routes were functions -- and the invariants.
void test_bwd_route() {
  struct Want { WgradKernel wg; DgradKernel dg; ConvForm dform; };
  // Default switches, fp32 plan, autocast off.  A data gradient is a stride-1 conv on the op's INPUT grid whatever the forward's stride
  // or upsampling (zero-stuffed dY; the upsampled grid, sum-pooled afterwards), so the stride-2 and upsample convs of these widths take
  // the Winograd kernel as well; the last conv's dY has 8 channels, which the Winograd kernel does not take.
  const Want want[RC_COUNT] = {
      /* WINO_FULL         */ {WG_WINO, DG_WINO, FORM_B6},
      /* WINO_FULL_SKIP    */ {WG_WINO, DG_WINO, FORM_B6},
      /* WINO_HALF         */ {WG_WINO, DG_WINO, FORM_B6},
      /* WINO_HALF_SKIP    */ {WG_WINO, DG_WINO, FORM_B6},
      /* QUARTER           */ {WG_ZS, DG_QR, FORM_B6},
      /* QUARTER_NO_TRAIN  */ {WG_ZS, DG_GENERIC, FORM_FP32},     // (the class of the CM_NO_TRAIN_QR switch: walked with it set)
      /* KSPLIT            */ {WG_GENERIC, DG_WINO, FORM_B6},
      /* STRIDE2           */ {WG_GENERIC, DG_WINO, FORM_B6},
      /* UPS_STATS         */ {WG_PAR, DG_WINO, FORM_B6},
      /* UPS_NO_STATS      */ {WG_PAR, DG_WINO, FORM_B6},
      /* FIRST             */ {WG_PACK, DG_NONE, FORM_FP32},
      /* LAST              */ {WG_PACK, DG_GENERIC, FORM_FP32},
      /* 1X1               */ {WG_1X1, DG_GENERIC, FORM_FP32},
      /* 1X1_STATS         */ {WG_1X1, DG_GENERIC, FORM_FP32},
      /* SKIP_ABSORBED     */ {WG_1X1, DG_GENERIC, FORM_FP32},
  };
  bool BwdKnobs::*const sw[] = {nullptr, &BwdKnobs::no_wino, &BwdKnobs::no_wino_b6, &BwdKnobs::no_train_b6, &BwdKnobs::no_train_qr,
                                &BwdKnobs::no_wino_wgrad, &BwdKnobs::no_wgrad_zsplit, &BwdKnobs::no_wgrad_pack, &BwdKnobs::no_wgrad_par,
                                &BwdKnobs::no_wgrad_1x1, &BwdKnobs::no_wgrad_zs_kernel};
  int walked = 0;
  for (int rc = 0; rc < RC_COUNT; ++rc)
    for (const int prec : {CM_PRECISION_F32, CM_PRECISION_F32X, CM_PRECISION_F16})   // (training refuses an f16 handle; the routes still answer)
      for (int ac = 0; ac < 2; ++ac)
        for (int frags = 0; frags < 2; ++frags)
          for (auto s : sw) {
            Op op = route_class_op(rc, prec);
            Act in, out;
            in.C = op.ca.C0; out.C = op.ca.out_cs; op.in0 = &in; op.out_act = &out;
            op.ref_taps = op.cls == K_CONV1 ? 1 : 27;
            BwdCtx ctx;
            ctx.precision = prec; ctx.autocast = ac; ctx.f16_frags = frags; ctx.max_batch = 2; ctx.in_channels = 3;
            if (rc == RC_FIRST) ctx.x8 = &in;
            BwdKnobs k;
            if (s) k.*s = true;
            if (rc == RC_QUARTER_NO_TRAIN_QR) k.no_train_qr = true;
            const BwdGeom g = bwd_geom(op, ctx, k);
            const WgradRoute w = wgrad_route(op, g, ctx, k);
            const DgradRoute d = dgrad_route(op, g, ctx, k);
            ++walked;
            // the table, then what each switch moves: exactly the rows it names, to the fallback the old else-branch reached
            Want e = want[rc];
            const bool f16 = ac && frags;
            ConvForm wform = (e.wg == WG_WINO && f16) ? FORM_F16 : FORM_FP32;
            if (e.dg == DG_WINO) e.dform = f16 ? FORM_F16 : prec == CM_PRECISION_F16 ? FORM_FP32 : FORM_B6;
            if (e.dg == DG_QR && prec == CM_PRECISION_F16) { e.dg = DG_GENERIC; e.dform = FORM_FP32; }   // (no six-term fragments on that plan)
            if (k.no_wino && e.dg == DG_WINO) { e.dg = DG_GENERIC; e.dform = FORM_FP32; }
            if ((k.no_wino_b6 || k.no_train_b6) && e.dform == FORM_B6 && e.dg == DG_WINO) e.dform = FORM_FP32;
            if (k.no_train_qr && e.dg == DG_QR) { e.dg = DG_GENERIC; e.dform = FORM_FP32; }
            if (k.no_wino_wgrad && e.wg == WG_WINO) { e.wg = WG_GENERIC; wform = FORM_FP32; }
            if ((k.no_wgrad_zsplit || k.no_wgrad_zs_kernel) && e.wg == WG_ZS) e.wg = WG_GENERIC;
            if (k.no_wgrad_pack && e.wg == WG_PACK) e.wg = WG_GENERIC;
            if (k.no_wgrad_par && e.wg == WG_PAR) e.wg = WG_GENERIC;
            if (k.no_wgrad_1x1 && e.wg == WG_1X1) e.wg = WG_GENERIC;
            EXPECT(w.kernel == e.wg && w.form == wform && d.kernel == e.dg && d.form == e.dform);
            // the invariants
            if (w.form == FORM_F16 || d.form == FORM_F16) EXPECT(ac && frags);
            EXPECT(w.form == FORM_FP32 || (w.form == FORM_F16 && w.kernel == WG_WINO));
            if (d.form == FORM_B6) EXPECT(prec != CM_PRECISION_F16);
            if (d.kernel == DG_QR) EXPECT(op.qr && op.d_wqr_b6 && d.form == FORM_B6);
            if (d.kernel == DG_WINO) EXPECT(dgrad_wino_ok(g, k) && cm::conv_wino_ok(g.da));
            EXPECT((d.kernel == DG_NONE) == (rc == RC_FIRST));
            EXPECT(g.zsplit == ((rc == RC_QUARTER || rc == RC_QUARTER_NO_TRAIN_QR) && !k.no_wgrad_zsplit));   // the z-split row order without its kernel: the generic one takes it
          }
  printf("test_bwd_route: %d combinations walked\n", walked);
}

// plan_backward on the op lists of host-only handles (cm_model_create with device = -1, then the list building of cm_model_finalize:
// "device" buffers are host memory nothing launches on).
struct HostList {
  cm_model *m = nullptr;
  BwdCtx ctx;
  explicit HostList(cm_unet_config c) {
    EXPECT(cm_model_create(&c, &m) == 0);
    EXPECT(dev_alloc(m, (void **)&m->tbuf, (size_t)c.max_batch * sizeof(long long)) == 0 && build_ops(m) == 0);
    for (Op &op : m->ops)
      if (op.kind == OP_CONV) EXPECT(resolve_conv(m, op) == 0);
    ctx = bwd_ctx(m);
  }
  ~HostList() { cm_model_destroy(m); }
};

// nparams < 0: whatever the handle holds.  refusal: the plan must say so in these words instead (a status for cm_train_init, no abort).
void check_bwd_plan(const HostList &h, int nparams, const char *refusal = nullptr) {
  const cm_model *m = h.m;
  const BwdKnobs k;
  const BwdPlan P = plan_backward(m->ops, h.ctx, k);
  if (refusal) { EXPECT(P.err.find(refusal) != std::string::npos); return; }
  if (nparams < 0) nparams = (int)m->params.size();
  EXPECT(P.err.empty() && P.ops.size() == m->ops.size());
  // every launching entry has both routes, and the text names each of them on a line of its own
  {
    int launching = 0;
    for (const BwdOp &e : P.ops) {
      const Op &op = m->ops[e.op];
      if (op.kind == OP_ATTN) { ++launching; EXPECT(cm::attn_bwd_limit(op.S, op.E, ATTN_HEADS) == nullptr); }
      if (op.kind != OP_CONV) continue;
      ++launching;
      EXPECT(e.wg.kernel >= WG_WINO && e.wg.kernel <= WG_GENERIC && e.dg.kernel >= DG_NONE && e.dg.kernel <= DG_GENERIC);
      EXPECT((e.dg.kernel == DG_NONE) == (op.in0 == h.ctx.x8));
      if (e.dg.kernel == DG_QR) EXPECT(train_qr_forms_ok(op, e.g));   // (the training forward takes conv_qr2 exactly there: no late refusal in run_conv_qr)
    }
    const std::string text = bwd_plan_text(m->ops, P, h.ctx.max_batch);
    EXPECT((int)std::count(text.begin(), text.end(), '\n') == launching && launching > 0);
  }
  // every gradient buffer: exactly one first writer, before every accumulator and before the entry that reads it as dY
  std::map<const Act *, int> first, reads;   // -> position in the plan
  std::map<const Act *, std::vector<int>> accs;
  for (int i = 0; i < (int)P.ops.size(); ++i) {
    const BwdOp &e = P.ops[i];
    const Op &op = m->ops[e.op];
    EXPECT(e.op == (int)m->ops.size() - 1 - i && &P.of(e.op) == &e);
    auto wrote = [&](const Act *a, bool acc) { if (acc) accs[a].push_back(i); else { EXPECT(!first.count(a)); first[a] = i; } };
    if (op.kind == OP_ATTN) { EXPECT(e.qa && e.oa && e.qa->d == op.qkv && e.oa->d == op.aout); reads[e.oa] = i; wrote(e.qa, false); }
    if (op.kind != OP_CONV) continue;
    reads[op.out_act] = i;
    if (op.resid_act) wrote(op.resid_act, e.acc_resid);
    if (e.dg.kernel == DG_NONE) continue;
    wrote(op.in0, e.acc_in0);
    if (op.in1 && e.tail != TAIL_POOL) wrote(op.in1, e.acc_in1);
  }
  for (auto &a : m->acts) {
    const Act *t = a.get();
    if (t == h.ctx.x8 || t == h.ctx.seed) { EXPECT(!first.count(t) && !accs.count(t)); continue; }   // data; the loss gradient's own buffer
    EXPECT(first.count(t) == 1 && reads.count(t) == 1);
    if (!first.count(t) || !reads.count(t)) continue;
    EXPECT(first[t] < reads[t]);
    for (int i : accs[t]) EXPECT(first[t] < i && i < reads[t]);
  }
  // the batch-sum pool: pairwise disjoint regions whose union is [0, reported size)
  std::vector<std::pair<size_t, size_t>> regions;
  for (const BwdOp &e : P.ops) {
    const Op &op = m->ops[e.op];
    if (op.kind != OP_CONV) continue;
    regions.push_back({e.bias_off, (size_t)h.ctx.max_batch * op.ca.Co});
    if (e.tail == TAIL_GN && e.dg.kernel != DG_NONE) regions.push_back({e.gn_off, (size_t)h.ctx.max_batch * 2 * (op.ca.C0 + op.ca.C1)});
  }
  std::sort(regions.begin(), regions.end());
  size_t end = 0;
  for (auto &r : regions) { EXPECT(r.first == end && r.second > 0); end = r.first + r.second; }
  EXPECT(end == P.pool_floats);
  for (const BwdSumJob &j : P.bsum) EXPECT(j.off + (size_t)(h.ctx.max_batch - 1) * j.stride + j.C <= P.pool_floats);
  // every trainable parameter's gradient is the destination of exactly one job or launch, the frozen sinusoid table of none
  std::map<std::string, int> dst;
  for (const BwdOp &e : P.ops) if (m->ops[e.op].kind == OP_CONV) ++dst[m->ops[e.op].wname];
  for (const BwdSumJob &j : P.bsum) ++dst[j.param];
  for (const BwdCopyJob &j : P.copy) ++dst[j.param];
  for (const char *n : {"time_embeddings.time_blocks.1.weight", "time_embeddings.time_blocks.1.bias", "time_embeddings.time_blocks.3.weight",
                        "time_embeddings.time_blocks.3.bias"}) ++dst[n];   // launch_time_bwd
  EXPECT((int)m->params.size() == nparams && (int)dst.size() == nparams - 1);
  for (const Param &p : m->params) EXPECT(dst.count(p.name) ? dst[p.name] == 1 : p.name == "time_embeddings.time_blocks.0.weight");
  // the copy jobs tile the stacked dense_1 gradients
  int off = 0;
  for (size_t i = 0; i < P.copy.size(); i += 2) {
    EXPECT(!P.copy[i].bias && P.copy[i + 1].bias && P.copy[i].off == off && P.copy[i + 1].off == off && P.copy[i].n == P.copy[i + 1].n * h.ctx.tx);
    off += (int)P.copy[i + 1].n;
  }
  EXPECT(off == m->nproj);
  // partial copies: at least one with the 256 MiB buffer, a clean failure without one
  for (const BwdOp &e : P.ops) {
    if (m->ops[e.op].kind != OP_CONV) continue;
    for (int B : {1, h.ctx.max_batch}) EXPECT(wgrad_groups(e, B, (size_t)64 << 20) >= 1);
    EXPECT(wgrad_groups(e, 1, 0) == 0 && std::string(cm_last_error()).find("partial buffer") != std::string::npos);
  }
  // autocast with the f16 fragments in place moves the Winograd layers' forms and nothing else
  BwdCtx ac = h.ctx; ac.autocast = ac.f16_frags = true;
  const BwdPlan Q = plan_backward(m->ops, ac, k);
  EXPECT(Q.err.empty() && Q.pool_floats == P.pool_floats && Q.ops.size() == P.ops.size());
  for (size_t i = 0; i < P.ops.size() && i < Q.ops.size(); ++i) {
    const BwdOp &a = P.ops[i], &b = Q.ops[i];
    EXPECT(a.wg.kernel == b.wg.kernel && a.dg.kernel == b.dg.kernel && a.bias_off == b.bias_off && a.gn_off == b.gn_off && a.acc_in0 == b.acc_in0);
    EXPECT(b.wg.form == (a.wg.kernel == WG_WINO ? FORM_F16 : FORM_FP32) && b.dg.form == (a.dg.kernel == DG_WINO ? FORM_F16 : a.dg.form));
  }
  // a list without its last conv: the op in front of it is an orphan, and the plan says so
  std::vector<Op> cut(m->ops.begin(), m->ops.end() - 1);
  int orphan = (int)cut.size() - 1;
  while (orphan >= 0 && cut[orphan].kind != OP_CONV && cut[orphan].kind != OP_ATTN) --orphan;
  const BwdPlan C = plan_backward(cut, h.ctx, k);
  EXPECT(!C.err.empty() && orphan >= 0 && C.err.find(cut[orphan].label) != std::string::npos);
}

void test_bwd_plan() {
  for (int C : {3, 4}) check_bwd_plan(HostList(atc_cfg(C, 12, 36, -1)), 169);   // ATC
  check_bwd_plan(HostList(atc_cfg(3, 28, 24, -1)), 169);                          // HERMES-CR-120
  check_bwd_plan(HostList(atc_cfg(3, 8, 20, -1)), 169);                           // the odd grid of tests/test_gpu_odd_grid.py
  check_bwd_plan(HostList(atc_cfg(3, 24, 72, -1)), 169);                          // attention scratch in a global slab
  {
    cm_unet_config c = atc_cfg(3, 4, 8, -1);                                      // the narrow model of the parity tests (base 8)
    c.base_channels = 8; c.max_batch = 3;
    check_bwd_plan(HostList(c), 169);
  }
  {
    HostList big(atc_cfg(3, 24, 72, -1)), atc(atc_cfg(3, 12, 36, -1));
    EXPECT(plan_backward(big.m->ops, big.ctx, BwdKnobs()).attn_floats > 0 && plan_backward(atc.m->ops, atc.ctx, BwdKnobs()).attn_floats == 0);
  }
}

// The geometries of tests/train_limit_cases.py (the rows that differ in dropout alone share a plan with "ethucy"): what a handle
// admits beyond the tuned grids.  Each is planned on a host-only handle and held to the same invariants; print: the plan's text.
// refusal: the words of the status instead -- "build: ..." from the list building of cm_model_finalize, anything else from plan_backward
struct LimitCase { const char *id; int rows, cols, past, future, C, base, levels, mult[4], att[4], res, B; const char *refusal; };
const LimitCase kLimitCases[] = {
    {"ethucy", 8, 12, 5, 3, 3, 32, 3, {1, 2, 4}, {0, 0, 1}, 1, 3, nullptr},
    {"hermes_bn", 28, 16, 5, 3, 3, 32, 3, {1, 2, 4}, {0, 0, 1}, 1, 3, nullptr},
    {"hermes_bo", 12, 24, 5, 3, 3, 32, 3, {1, 2, 4}, {0, 0, 1}, 1, 2, nullptr},
    {"hermes_cr90", 12, 20, 5, 3, 3, 32, 3, {1, 2, 4}, {0, 0, 1}, 1, 3, nullptr},
    {"ethucy_b9", 8, 12, 5, 3, 3, 32, 3, {1, 2, 4}, {0, 0, 1}, 1, 9, nullptr},
    {"grid4x4", 4, 4, 5, 3, 3, 32, 3, {1, 2, 4}, {0, 0, 1}, 1, 1, nullptr},
    {"plane64", 32, 32, 5, 3, 3, 32, 3, {1, 2, 4}, {0, 0, 1}, 1, 1, nullptr},
    {"plane72", 48, 24, 5, 3, 3, 32, 3, {1, 2, 4}, {0, 0, 1}, 1, 1, nullptr},
    {"attn_half", 16, 32, 5, 3, 3, 32, 3, {1, 2, 4}, {0, 1, 1}, 1, 1, nullptr},
    {"attn_half640", 16, 40, 5, 3, 3, 32, 3, {1, 2, 4}, {0, 1, 1}, 1, 1, "too many tokens"},
    {"frames4", 8, 12, 3, 1, 3, 32, 3, {1, 2, 4}, {0, 0, 1}, 1, 2, nullptr},
    {"frames12", 8, 12, 8, 4, 3, 32, 3, {1, 2, 4}, {0, 0, 1}, 1, 2, nullptr},
    {"base8", 8, 12, 5, 3, 3, 8, 3, {1, 2, 4}, {0, 0, 1}, 1, 2, nullptr},
    {"base16", 8, 12, 5, 3, 3, 16, 3, {1, 2, 4}, {0, 0, 1}, 1, 2, nullptr},
    {"base24", 8, 12, 5, 3, 3, 24, 3, {1, 2, 4}, {0, 0, 1}, 1, 2, "build: head width"},
    {"ch1", 8, 12, 5, 3, 1, 32, 3, {1, 2, 4}, {0, 0, 1}, 1, 2, nullptr},
    {"ch4", 8, 12, 5, 3, 4, 32, 3, {1, 2, 4}, {0, 0, 1}, 1, 2, nullptr},
    {"ch5", 8, 12, 5, 3, 5, 32, 3, {1, 2, 4}, {0, 0, 1}, 1, 2, nullptr},
    {"ch8", 8, 12, 5, 3, 8, 32, 3, {1, 2, 4}, {0, 0, 1}, 1, 2, nullptr},
    {"res2", 8, 12, 5, 3, 3, 32, 3, {1, 2, 4}, {0, 0, 1}, 2, 2, nullptr},
    {"levels2", 8, 12, 5, 3, 3, 32, 2, {1, 2}, {0, 1}, 1, 2, nullptr},
    {"levels4", 8, 16, 5, 3, 3, 32, 4, {1, 2, 2, 4}, {0, 0, 0, 1}, 1, 2, nullptr},
    {"mult112", 8, 12, 5, 3, 3, 32, 3, {1, 1, 2}, {0, 0, 1}, 1, 2, nullptr},
};
cm_unet_config limit_cfg(const LimitCase &t) {
  cm_unet_config c{};
  c.in_channels = c.out_channels = t.C;
  c.num_res_blocks = t.res; c.base_channels = t.base; c.n_levels = t.levels;
  for (int i = 0; i < t.levels; ++i) { c.channel_mult[i] = t.mult[i]; c.apply_attention[i] = t.att[i]; }
  c.time_multiple = 4; c.rows = t.rows; c.cols = t.cols; c.past_len = t.past; c.future_len = t.future; c.max_batch = t.B; c.device = -1;
  return c;
}
void test_bwd_plan_limits(bool print) {
  for (const LimitCase &t : kLimitCases) {
    if (t.refusal && !strncmp(t.refusal, "build: ", 7)) {   // no op list: the handle itself is refused, by name
      cm_unet_config c = limit_cfg(t);
      cm_model *m = nullptr;
      EXPECT(cm_model_create(&c, &m) == 0 && dev_alloc(m, (void **)&m->tbuf, sizeof(long long)) == 0);
      EXPECT(build_ops(m) != 0 && strstr(cm_last_error(), t.refusal + 7));
      if (print) printf("== %s: %s\n", t.id, cm_last_error());
      cm_model_destroy(m);
      continue;
    }
    HostList h(limit_cfg(t));
    check_bwd_plan(h, -1, t.refusal);
    if (!print) continue;
    const BwdPlan P = plan_backward(h.m->ops, h.ctx, BwdKnobs());
    printf("== %s%s%s\n%s", t.id, P.err.empty() ? "" : ": ", P.err.c_str(), P.err.empty() ? bwd_plan_text(h.m->ops, P, h.ctx.max_batch).c_str() : "");
  }
  printf("test_bwd_plan_limits: %zu geometries planned\n", sizeof kLimitCases / sizeof kLimitCases[0]);
}

}  // namespace

int main(int argc, char **argv) {
  if (argc > 1 && std::string(argv[1]) == "plans") { test_bwd_plan_limits(true); return 0; }   // the limit geometries' backward plans, as text
  test_bwd_route();
  test_bwd_plan();
  test_bwd_plan_limits(false);
  test_opt_store();
  test_schedule();
  test_plan_and_params();
  test_packers();
  test_fragment_digests();
  test_value_index_layouts();
  test_tile_planner();
  test_round3_packers();
  test_wino_form_dispatch();
  test_conv_route();
  test_forward_plan();
  test_loop_ends();
  test_misc_errors();
  printf("selftest ok: %d checks\n", g_checks);
  return 0;
}
