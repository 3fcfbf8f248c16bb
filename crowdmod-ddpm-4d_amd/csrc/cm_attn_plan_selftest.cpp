// Host-side self-test of the attention block's place in the forward plan (plan_forward: OpPlan::attn_sample), built by `make asan`
// next to cm_host_selftest and run under ASan / UBSan as a stand-alone program: no kernel is launched, no device is needed.
// Hand-built op lists -- a fused attention block and the GroupNorm finalisation behind it -- through the four precision plans x
// inference / training, stale fragments, the token counts at the kernel's limit, missing fragments and a planned carry; each case
// checks which launch the block takes, whether its second pass carries the finalisation, and the statistics slots written.
#include "cm_model.cpp"

#include <cstdio>
#include <memory>

namespace {

int failures = 0;
#define EXPECT(cond)                                                                  \
  do {                                                                                \
    if (!(cond)) { fprintf(stderr, "%s:%d: EXPECT(%s) failed\n", __FILE__, __LINE__, #cond); ++failures; } \
  } while (0)

struct List {
  std::vector<std::unique_ptr<Act>> acts;
  std::vector<Op> ops;
  Act *act(int C, int Z, int Y, int X) {
    static float buf[4];
    acts.push_back(std::make_unique<Act>());
    Act *a = acts.back().get();
    a->C = C; a->Z = Z; a->Y = Y; a->X = X; a->part = a->cnt = buf;
    return a;
  }
};

// [0] the fused block on S = 2 Y X tokens, [1] the finalisation of its output: left to a whole-sample quarter-resolution consumer
// (qr: FIN_QR, as in every sampling plan) or free for the block's second pass to carry
List block_list(int Y, int X, bool frags, bool qr, bool with_fin = true) {
  static float frag[4];
  List L;
  Act *x = L.act(128, 2, Y, X), *o = L.act(128, 2, Y, X);
  Op fb;
  fb.kind = OP_ATTNBLK; fb.cls = K_ATTN; fb.label = "attention (fused block)";
  fb.ab_x = x; fb.ab_out = o; fb.S = 2 * Y * X; fb.E = 128;
  if (frags) { fb.d_win_h2 = fb.d_wout_h2 = frag; fb.ab_in_oscale = fb.ab_out_oscale = 0.25f; }
  L.ops.push_back(fb);
  if (with_fin) {
    Op g;
    g.kind = OP_GNFIN; g.cls = K_NORM; g.g0 = o; g.label = "gn"; g.qr_consumer = qr;
    L.ops.push_back(g);
  }
  return L;
}

FwdCtx ctx_of(int precision, bool train, bool stale = false, int B = 2) {
  FwdCtx c;
  c.precision = precision; c.train_fwd = train; c.h2_stale = stale; c.B = B;
  return c;
}

void test_attention_plan() {
  const int plans[4] = {CM_PRECISION_F32, CM_PRECISION_F32X, CM_PRECISION_F32R, CM_PRECISION_F16};
  int cases = 0;
  for (int prec : plans) {
    // inference, 54 tokens, the consumer finalises: the whole-sample launch on the default plan only
    {
      const List L = block_list(3, 9, true, true);
      const FwdPlan P = plan_forward(L.ops, ctx_of(prec, false));
      EXPECT(P.err.empty() && P.ops[0].launch && P.ops[0].ns_out == 2 && P.ops[0].carries == -1);
      EXPECT(P.ops[0].attn_sample == (prec == CM_PRECISION_F32));
      EXPECT(P.ops[1].fin == FIN_QR && !P.ops[1].launch && P.ops[1].ns0 == 2);
      EXPECT(plan_forward(L.ops, ctx_of(prec, false, false, 64)).ops[0].attn_sample == (prec == CM_PRECISION_F32));   // any batch
      ++cases;
    }
    // training forward: the block is not of that context -- nothing launched, no slots written
    {
      const List L = block_list(3, 9, true, true, false);
      const FwdPlan P = plan_forward(L.ops, ctx_of(prec, true));
      EXPECT(P.err.empty() && !P.ops[0].launch && !P.ops[0].attn_sample && P.ops[0].ns_out == 0 && P.ops[0].carries == -1);
      ++cases;
    }
    // a planned carry: the second pass finalises the consumer's GroupNorm, so the two launches stay
    {
      const List L = block_list(3, 9, true, false);
      const FwdPlan P = plan_forward(L.ops, ctx_of(prec, false));
      EXPECT(P.err.empty() && P.ops[0].launch && P.ops[0].carries == 1 && !P.ops[0].attn_sample && P.ops[0].ns_out == 2);
      EXPECT(P.ops[1].fin == FIN_COMBINE && !P.ops[1].launch && P.ops[1].ns0 == 2);
      ++cases;
    }
  }
  // fragments an optimizer step has left behind: the two launches until refresh_h2
  {
    const List L = block_list(3, 9, true, true);
    const FwdPlan P = plan_forward(L.ops, ctx_of(CM_PRECISION_F32, false, true));
    EXPECT(P.err.empty() && P.ops[0].launch && !P.ops[0].attn_sample && P.ops[0].ns_out == 2 && P.ops[1].fin == FIN_QR);
    ++cases;
  }
  // no fragments (another plan's handle), a weight without a scale
  {
    List L = block_list(3, 9, false, true);
    EXPECT(!plan_forward(L.ops, ctx_of(CM_PRECISION_F32, false)).ops[0].attn_sample);
    L = block_list(3, 9, true, true);
    L.ops[0].ab_out_oscale = 0.f;
    EXPECT(!plan_forward(L.ops, ctx_of(CM_PRECISION_F32, false)).ops[0].attn_sample);
    L.ops[0].ab_out_oscale = 0.25f; L.ops[0].ab_in_oscale = 0.f;
    EXPECT(!plan_forward(L.ops, ctx_of(CM_PRECISION_F32, false)).ops[0].attn_sample);
    cases += 3;
  }
  // token counts: 2 (one slot), 32 / 34 (one / two slots), 64 (the last admitted), 66 (three slots, the two launches)
  {
    struct T { int Y, X, S, ns; bool taken; };
    const T tok[] = {{1, 1, 2, 1, true}, {4, 4, 32, 1, true}, {1, 17, 34, 2, true}, {4, 8, 64, 2, true}, {1, 33, 66, 3, false}, {3, 14, 84, 3, false}};
    for (const T &t : tok) {
      const List L = block_list(t.Y, t.X, true, true);
      const FwdPlan P = plan_forward(L.ops, ctx_of(CM_PRECISION_F32, false));
      EXPECT(L.ops[0].S == t.S && P.err.empty() && P.ops[0].launch && P.ops[0].ns_out == t.ns && P.ops[1].ns0 == t.ns);
      EXPECT(P.ops[0].attn_sample == t.taken && cm::attn_sample_ok(t.S, 128, ATTN_HEADS, GN_GROUPS) == t.taken);
      ++cases;
    }
    EXPECT(!cm::attn_sample_ok(0, 128, ATTN_HEADS, GN_GROUPS) && !cm::attn_sample_ok(65, 128, ATTN_HEADS, GN_GROUPS));
    EXPECT(!cm::attn_sample_ok(54, 64, ATTN_HEADS, GN_GROUPS) && !cm::attn_sample_ok(54, 128, 8, GN_GROUPS) && !cm::attn_sample_ok(54, 128, ATTN_HEADS, 4));
    EXPECT(cm::attn_sample_lds_bytes() <= 160 * 1024);
  }
  // the launcher refuses what the plan must never hand it (before any launch)
  {
    cm::AttnSampleArgs a{};
    a.B = 2; a.S = 66; a.nslots = 3;
    EXPECT(cm::launch_attn_sample(a, nullptr) == hipErrorInvalidValue);
    a.S = 54; a.nslots = 2;                            // no fragments
    EXPECT(cm::launch_attn_sample(a, nullptr) == hipErrorInvalidValue);
    ++cases;
  }
  // the fragment pack: lane order and the two terms of one element
  {
    std::vector<float> w((size_t)32 * 64);
    for (size_t i = 0; i < w.size(); ++i) w[i] = (float)((int)(i % 97) - 48) * 0.0131f;
    const float ws = h2_wscale(w.data(), w.size());
    const std::vector<float> f = pack_attn_h2(w.data(), 32, 64, ws);
    EXPECT(f.size() == (size_t)32 * 64);                // two halves per float, two terms per element
    const uint16_t *h = reinterpret_cast<const uint16_t *>(f.data());
    const int n = 21, k = 45, cb = n / 16, ks = k / 32, lane = 16 * ((k % 32) / 8) + n % 16, i = k % 8;
    const float hi = f16_bits_to_f32(h[((((size_t)cb * 2 + ks) * 2 + 0) * 64 + lane) * 8 + i]);
    const float mid = f16_bits_to_f32(h[((((size_t)cb * 2 + ks) * 2 + 1) * 64 + lane) * 8 + i]);
    const float v = w[(size_t)n * 64 + k] * ws;
    EXPECT(std::fabs(hi + mid - v) <= std::ldexp(std::fabs(v), -21));
    ++cases;
  }
  printf("test_attention_plan: %d cases\n", cases);
}

}  // namespace

int main() {
  test_attention_plan();
  if (failures) { fprintf(stderr, "%d failure(s)\n", failures); return 1; }
  printf("attention plan selftest ok\n");
  return 0;
}
