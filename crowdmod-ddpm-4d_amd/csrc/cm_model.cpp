// Host side of libcrowdmod_hip.so: model construction (mirrors the reference UNet
// constructor, /root/reference/models/backbones/unet.py:11-122), weight packing
// into MFMA fragment order, the launch sequence of one UNet forward
// (unet.py:124-167, layers.py:55-78,12-18) and the on-device reverse loops
// (models/diffusion/ddpm.py:206-282).  Everything here is plain C++ over the HIP
// runtime; the public surface is the C ABI in include/crowdmod_hip.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <numeric>
#include <set>
#include <string>
#include <thread>
#include <vector>

#include "../../include/crowdmod_hip.h"
#include "cm_kernels.h"
#include "cm_pack.h"

using namespace cm_pack;

namespace {

thread_local std::string g_err;

int fail(const char *fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return 1;
}

#define CM_HIP(expr)                                                                      \
  do {                                                                                    \
    hipError_t _e = (expr);                                                               \
    if (_e != hipSuccess) return fail("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
  } while (0)

constexpr int GN_GROUPS = 8;       // layers.py:9,30,41 ; unet.py:119
constexpr float GN_EPS = 1e-5f;
constexpr int ATTN_HEADS = 4;      // layers.py:10
constexpr int TIME_ROWS = 1000;    // embeddings.py:7
constexpr int MAX_SLICES = 16;
constexpr int MAX_SLOTS = 512;  // statistics slots per sample (32-row accumulator blocks of a conv)

enum KClass { K_CONV3 = 0, K_CONV1 = 1, K_NORM = 2, K_ATTN = 3, K_ELEM = 4, K_NCLASS = 8 };

struct Param {
  std::string name;
  std::vector<int64_t> shape;
  std::vector<float> host;
  bool set = false;
  int64_t numel() const {
    int64_t n = 1;
    for (auto s : shape) n *= s;
    return n;
  }
};

// A channels-last activation [B][Z][Y][X][C] plus its per-channel statistics partials.
struct Act {
  std::string name;
  float *d = nullptr;
  float *g = nullptr;     // gradient buffer (training)
  int C = 0, Z = 0, Y = 0, X = 0;
  float *part = nullptr;  // [B][slots][C][2] per-slot (mean, M2) of every channel; the slot count is the producer's, a fact of
  float *cnt = nullptr;   // [B][slots] rows behind each slot                          the forward's plan (plan_forward)
  int nslice = 1;         // slots when the stand-alone statistics kernel fills them
  bool h16 = false;       // reduced-precision plan: the tensor is stored as _Float16 (same layout and strides; plan_h16)
  int V() const { return Z * Y * X; }
};

struct BlockDesc {
  int kind;  // 0 res, 1 down, 2 up
  std::string prefix;
  int cin, cout, attention, skip, level;
};

enum OpKind { OP_CONV, OP_STATS, OP_GNFIN, OP_ATTN, OP_ATTNBLK };

struct Op {
  OpKind kind;
  int cls;
  // conv
  cm::ConvArgs ca{};
  int MB = 1, NB = 1;         // tile geometry (ca.bs .. ca.ntx, MB) and tables: resolve_conv, at finalize
  int *d_hvtab = nullptr, *d_mtab = nullptr;  // device copies of the box coordinate tables
  Act *stat_act = nullptr;  // output tensor whose GroupNorm statistics this conv produces in its epilogue
  int pm_off = -1;          // >= 0: conv_2 of a ResnetBlock; offset of its Dropout3d mask row slice (training forward)
  const Act *in0 = nullptr, *in1 = nullptr;  // forward inputs (for the backward pass)
  std::string wname, bname;
  int temb_off = -1;        // >= 0: slice of the time-embedding projection added in the epilogue
  int gn_op = -1;           // index of the OP_GNFIN op that produced this conv's on-load normalisation
  int ref_taps = 1;         // taps of the reference weight (27 even when the forward runs the 8-tap parity form)
  int ks = 1;               // K split over workgroups (tiny-spatial layers) + combine pass
  // inference-time fusion of the block's 1x1x1 skip conv into conv_2 (see ConvArgs::s2w)
  const Act *skip0 = nullptr, *skip1 = nullptr;
  std::string skip_w, skip_b;
  float *d_s2w = nullptr, *d_bias_fused = nullptr;
  bool skip_if_fused = false;  // this op is the stand-alone skip conv that a later op absorbs
  bool wino = false;        // Winograd F(2x2,3x3) kernel (cm_conv_wino.hip): full- and half-resolution stride-1 3x3x3 layers.  add_conv
                            //   sets it from the layer shape; resolve_conv withdraws it when the tile does not fit; final after finalize
  float *d_wwino = nullptr;
  float *d_wwino16 = nullptr;   // the same weights as f16 operands (reduced-precision plan, cm_model_set_precision)
  float *d_wwino16t = nullptr;  // ... of a default-plan handle that trains under autocast (cm_train_set_autocast): re-packed after every update
  float *d_wwino_b6 = nullptr;  // fp32 plan, inference forward, two-tile layers: exact bf16 x 3 split of d_wwino (pack_wino_b6)
  long long wwino_floats = 0;   // element count of d_wwino
  float *d_wfrag16 = nullptr;   // f16 fragments of a parity-form upsample conv (reduced-precision plan)
  float *d_w1x1_16 = nullptr;   // f16 fragments of a 1x1x1 conv without statistics (pack_1x1_f16; reduced-precision plan, inference)
  long long wpar_stride16 = 0;
  bool f16d = false;        // reduced-precision plan: direct f16-operand kernel (cm_conv_f16.hip) instead of the Winograd one
  int f16d_bz = 0, f16d_by = 0, f16d_bx = 0, f16d_mbw = 0;
  bool ups = false;         // parity-form upsample conv on the stage-once kernel (cm_conv_ups.hip); source tile + row blocks per wave
  int ups_tz = 0, ups_ty = 0, ups_tx = 0, ups_mbw = 0, ups_planes = 0;
  float *d_wups16 = nullptr;    // its f16 fragments under the reduced-precision plan (pack_ups_f16), floats per parity class
  long long wups16_stride = 0;
  float *d_wups_b6 = nullptr;   // fp32 plan, inference forward: bf16 x 3 split fragments (pack_ups_b6) for the six-term products
  long long wups_b6_stride = 0;
  float *d_w16d = nullptr, *d_w16d_skip = nullptr;
  bool h2_off = false;      // refresh_h2: this layer's GroupNorm affine no longer satisfies the static bound -> six-term form
  bool dbg_h2 = false;      // cm_debug_conv_io mode 2: raw sources, but the h2 form where the plan has one (the caller bounds its operands)
  bool dbg_raw = false;     // cm_debug_conv_io: the whole-sample quarter-resolution kernel without its GroupNorm (raw sources)
  // default plan, layers whose input is GroupNorm + SiLU output (bounded): f16 two-way splits, three cross terms ("h2", cm_kernels.h:
  // cm_split2_f16) instead of bf16 three-way splits, six cross terms -- same accuracy, half the matrix instructions.  Fragments of
  // w * 2^k; h2_oscale = 2^-k.  Inference-only handles (a handle that trains keeps the six-term form: its repack kernels do not
  // maintain these fragments).
  float *d_wfin_h2 = nullptr, *d_wwino_h2 = nullptr, *d_wqr_h2 = nullptr;
  float *d_wups_h2 = nullptr;   // upsample conv (raw source): h2 with a per-sample scale from the source tensor's slot statistics
  float h2_oscale = 1.f;
  bool qr = false;         // whole-sample kernel of the lowest resolution (cm_conv_qr.hip), inference plan
  float *d_wqr = nullptr, *d_wqr_skip = nullptr;
  float *d_wqr_b6 = nullptr;    // exact bf16 x 3 split of d_wqr for the six-term form of conv_qr2 (pack_qr_b6)
  bool train_qr = false;        // the training forward may take conv_qr2 as well (set by train_setup once the geometry is checked)
  long long wqr_floats = 0;
  bool qr_consumer = false; // OP_GNFIN whose only consumer is a qr conv: that kernel finalises the statistics itself
  bool first_k = false;     // the UNet's first conv on its dedicated kernel (cm_conv_io.hip); resolve_conv withdraws it when no tile fits
  int first_cin = 4;        //   input channels it contracts per tap: 4 (C <= 4) or 8
  float *d_wfirst = nullptr;
  bool small_n = false;     // <= 8 output channels: vector-ALU kernel (cm_conv_small.hip)
  float *d_wsmall = nullptr;
  int small_nco = 4;
  bool fin = false;         // the last conv on the matrix core, taps packed into the columns (cm_conv_fin.hip); falls back to small_n
  int fin_by = 0, fin_bx = 0;
  float *d_wfin = nullptr, *d_wfin16 = nullptr, *d_wfin_src = nullptr;   // six-term / f16 fragments; device copy of the reference-layout weights
  float *d_zero_bias = nullptr;
  const Act *out_act = nullptr, *resid_act = nullptr;
  double flops_per_sample = 0;
  std::string label;
  double prof_ms = 0;
  int64_t prof_n = 0;
  // stats
  const Act *act = nullptr;
  // gn finalize
  const Act *g0 = nullptr, *g1 = nullptr;
  const float *gamma = nullptr, *beta = nullptr;
  float *gn_out = nullptr;
  float *gn_mr = nullptr;   // [B][2][Ct] group mean / rstd per channel (allocated when training)
  std::string gname, bename;  // state_dict names of gamma / beta
  // attention
  const float *qkv = nullptr;
  float *aout = nullptr;
  int S = 0, E = 0;
  // fused attention block (inference plan): replaces the four ops flagged `in_attn_block` in front of it
  bool in_attn_block = false;
  const Act *ab_x = nullptr;      // block input (and residual)
  Act *ab_out = nullptr;          // block output (statistics producer)
  int ab_gn = -1, ab_qkv = -1, ab_outc = -1;   // indices of the ops whose device parameters it reads
  float *d_win = nullptr, *d_wout = nullptr;   // reference-layout copies of in_proj_weight / out_proj.weight
  std::string win_name, wout_name;
  // default plan, S <= 64: the block as one whole-sample launch (attn_sample_kernel) on h2 fragments of the two weights
  // (pack_attn_h2 of w * 2^k; ab_*_oscale = 2^-k, 0 = no fragments: all-zero or non-finite weights)
  float *d_win_h2 = nullptr, *d_wout_h2 = nullptr;
  float ab_in_oscale = 0.f, ab_out_oscale = 0.f;
};

enum ConvKernel { CONV_NONE, CONV_QR, CONV_KSPLIT, CONV_UPS, CONV_F16D, CONV_WINO, CONV_FIRST, CONV_FIN, CONV_SMALLN, CONV_1X1_F16, CONV_GENERIC };
const char *const kConvKernelName[] = {"none", "qr", "ksplit", "ups", "f16d", "wino", "first", "fin", "smalln", "1x1_f16", "generic"};
// (= ConvArgs::f16 where a kernel takes it)  fp32 matrix instructions; f16 operands; six bf16 cross terms of exact three-way splits;
// their three leading terms (relaxed plan); three f16 cross terms of two-way splits ("h2", bounded operands)
enum ConvForm { FORM_FP32 = 0, FORM_F16 = 1, FORM_B6 = 2, FORM_B3 = 3, FORM_H2 = 4 };
struct ConvRoute { ConvKernel kernel; ConvForm form; };

// The plan of one forward (plan_forward).  B: the batch of ONE enqueue (a lane's share); only conv_wino_p_taken under the f16 plan reads it
struct FwdCtx { int precision = CM_PRECISION_F32; bool train_fwd = false, h2_stale = false; int B = 1; bool autocast = false; };   // autocast: the training forward of a handle in cm_train_set_autocast mode 1
// Who turns the slot statistics behind an OP_GNFIN into scale / shift rows, in order of precedence: its whole-sample quarter-resolution
// consumer; the second pass of the K-split conv / attention block that produces g0; its Winograd consumer (few slots); its own launch
enum FinBy { FIN_NONE, FIN_QR, FIN_COMBINE, FIN_WINO, FIN_ALONE };
struct OpPlan {
  bool launch = false;       // the op enqueues something in this context
  ConvRoute route{CONV_NONE, FORM_FP32};
  int ns_out = 0;            // statistics slots per sample this op writes (conv: stat_act; OP_STATS: act; OP_ATTNBLK: ab_out), 0 = none
  int ns0 = 0, ns1 = 0;      // slots of the statistics behind it: OP_GNFIN g0 / g1 (whoever finalises reads them here); conv: in0 (h2 upsample form)
  FinBy fin = FIN_NONE;      // OP_GNFIN of this context
  int carries = -1;          // K-split conv / attention block: the OP_GNFIN its second pass finalises (FIN_COMBINE)
  bool attn_sample = false;  // OP_ATTNBLK: one whole-sample launch (attn_sample_kernel) instead of the head launch + combine
};
struct FwdPlan { FwdCtx ctx; std::vector<OpPlan> ops; std::string err; };   // one entry per op; err: the list cannot run in this context

}  // namespace

struct cm_schedule {
  int T = 0;
  int device = 0;
  std::vector<float> tab[6];
  float *d_sab = nullptr, *d_s1m = nullptr;
};

struct cm_train_state;
struct cm_dit_plan;   // cm_dit_host.inc: the DiT4D_V4 or DiT2D backbone (null on a UNet handle)
void cm_free_train_state(cm_train_state *t);  // cm_train_host.inc (host-side struct only; device buffers live in allocs)
struct cm_model {
  cm_unet_config cfg{};   // DiT handle: the sampler geometry (channels, grid, frames, max_batch, device) only
  cm_dit_plan *dit = nullptr;
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t lane_stream[4] = {nullptr, nullptr, nullptr, nullptr};  // extra lanes of the batch interleave
  hipEvent_t ev_join[4] = {nullptr, nullptr, nullptr, nullptr}, ev_fork = nullptr;
  std::vector<Param> params;
  std::map<std::string, int> pindex;
  std::vector<BlockDesc> enc, bott, dec;
  int final_ch = 0;
  bool finalized = false;
  int precision = CM_PRECISION_F32;   // matrix-core operand type of the Winograd layers (inference plan)

  std::vector<void *> allocs;
  std::vector<std::unique_ptr<Act>> acts;
  std::map<std::string, Act *> act_by_name;
  std::vector<Op> ops;
  FwdPlan plan;           // of the last forward: assigned by the entry point on the calling thread; the launches and debug hooks only read it
  std::map<std::string, float *> dparam;  // raw uploaded small tensors

  // persistent device buffers
  float *x8 = nullptr;          // UNet input [B][L][H][W][8]
  Act *x8_act = nullptr;
  float *eps_cl = nullptr;      // UNet output channels-last [B][L][H][W][8]
  long long *tbuf = nullptr;    // [B] timestep per sample
  float *temb_table = nullptr;  // [1000][nproj]
  int nproj = 0;
  float *d_time[7] = {nullptr};  // device copies: table, W1, b1, W2, b2, Wd_all, bd_all
  struct cm_train_state *train = nullptr;
  float *dropmask = nullptr;    // [B][nproj] Dropout3d keep-mask/(1-p) of the current training forward
  // h2 fragments are built from the weights at load time; an optimizer step leaves them behind (the device repack kernels maintain
  // the bf16 fragments only).  Stale => the inference forward runs the six-term form; the next inference entry point re-derives them
  // from the master weights (refresh_h2, cm_train_host.inc) -- once per train -> sample transition.
  bool h2_stale = false;
  // training step: time-embedding projections of the batch computed from the live weights
  float *train_temb = nullptr;  // [B][nproj], row b
  long long *train_iota = nullptr;
  bool use_train_temb = false;
  bool train_autocast = false;   // cm_train_set_autocast mode 1: the training forward's Winograd layers on f16 operands (FwdCtx::autocast)
  float *mse_partial = nullptr, *mse_loss = nullptr;
  float *ks_scratch = nullptr;  // raw partial outputs of K-split convs [S][B][V][Co]
  size_t ks_scratch_floats = 0;
  float *xstate = nullptr;      // sampler state [B,C,H,W,F]
  cm::StepRow *d_steptab = nullptr;  // per-step scalars of the current loop (graph replay)
  size_t steptab_cap = 0;
  int *d_kctr = nullptr;        // device-side step counter read by the table-driven step kernels
  int *d_nonfinite = nullptr;   // result word of the sampler-output health check
  // What cm_sample_loop may leave out at the two ends of the UNet (loop_ends_plan): 1 the last conv computes the future planes only,
  // 2 it applies the sampler update in its tail (no sampler_step_kernel launch), 4 steps after the first launch only the first conv's
  // z tiles that see a future frame, 8 (measurements) the update runs on the thread that finishes a voxel.  0 = whole convs and a
  // separate sampler launch (cm_debug_loop_ends: tests compare the two sequences bit for bit in one process; CM_LOOP_ENDS under
  // CM_DIAG=1 sets a new handle's mask for A/B runs).
  int loop_ends = cm::diag_env("CM_LOOP_ENDS") ? (atoi(cm::diag_env("CM_LOOP_ENDS")) & 15) : 7;
  float *mass_q = nullptr;      // mass_preservation guidance quotient [max_batch,3,H,W,F] (allocated on first use)
  float *stage_past = nullptr, *stage_fut = nullptr, *stage_out = nullptr;  // host-variant staging
  float *stage_noise = nullptr;
  size_t stage_noise_cap = 0;
  float *stage_hist = nullptr;
  size_t stage_hist_cap = 0;

  // profiling
  bool profile = false;
  float prof_ms[K_NCLASS] = {0};
  int64_t prof_n[K_NCLASS] = {0};
  std::vector<std::pair<int, std::pair<hipEvent_t, hipEvent_t>>> prof_events[4];   // per batch lane (each lane's thread appends to its own)
  hipEvent_t prof_base = nullptr;                 // time origin of a profiled call (recorded on the call's stream)
  int prof_B = 0;                                 // batch of one enqueue of the profiled call (profile report)
  float prof_union_ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // per class: length of the UNION of its launch intervals over all lanes

  int L() const { return cfg.past_len + cfg.future_len; }
  int64_t per_sample() const { return (int64_t)cfg.in_channels * cfg.rows * cfg.cols * cfg.future_len; }
};

namespace {
int refresh_h2(cm_model *m);   // cm_train_host.inc: h2 fragments from the master weights of a handle that has trained

// ------------------------------------------------------------------------------
// construction
// ------------------------------------------------------------------------------
void add_param(cm_model *m, const std::string &name, std::vector<int64_t> shape) {
  Param p;
  p.name = name;
  p.shape = std::move(shape);
  p.host.assign((size_t)p.numel(), 0.f);
  m->pindex[name] = (int)m->params.size();
  m->params.push_back(std::move(p));
}

// Block wiring and state_dict names: same loop structure as unet.py:45-115.
void build_plan(cm_model *m) {
  const cm_unet_config &c = m->cfg;
  const int base = c.base_channels, nres = c.n_levels;
  const int64_t te = base, tx = (int64_t)base * c.time_multiple;
  add_param(m, "time_embeddings.time_blocks.0.weight", {TIME_ROWS, te});
  add_param(m, "time_embeddings.time_blocks.1.weight", {tx, te});
  add_param(m, "time_embeddings.time_blocks.1.bias", {tx});
  add_param(m, "time_embeddings.time_blocks.3.weight", {tx, tx});
  add_param(m, "time_embeddings.time_blocks.3.bias", {tx});
  add_param(m, "first.weight", {base, c.in_channels, 3, 3, 3});
  add_param(m, "first.bias", {base});

  std::vector<int> stack{base};
  int cin = base, idx = 0;
  for (int level = 0; level < nres; ++level) {
    const int cout = base * c.channel_mult[level];
    for (int r = 0; r < c.num_res_blocks; ++r) {
      m->enc.push_back({0, "encoder_blocks." + std::to_string(idx++), cin, cout, c.apply_attention[level] != 0, 0, level});
      cin = cout;
      stack.push_back(cin);
    }
    if (level != nres - 1) {
      m->enc.push_back({1, "encoder_blocks." + std::to_string(idx++), cin, cin, 0, 0, level});
      stack.push_back(cin);
    }
  }
  m->bott.push_back({0, "bottleneck_blocks.0", cin, cin, 1, 0, nres - 1});
  m->bott.push_back({0, "bottleneck_blocks.1", cin, cin, 0, 0, nres - 1});
  idx = 0;
  for (int level = nres - 1; level >= 0; --level) {
    const int cout = base * c.channel_mult[level];
    for (int r = 0; r < c.num_res_blocks + 1; ++r) {
      const int skip = stack.back();
      stack.pop_back();
      m->dec.push_back({0, "decoder_blocks." + std::to_string(idx++), skip + cin, cout, c.apply_attention[level] != 0, skip, level});
      cin = cout;
    }
    if (level != 0) m->dec.push_back({2, "decoder_blocks." + std::to_string(idx++), cin, cin, 0, 0, level});
  }
  m->final_ch = cin;

  auto add_block_params = [&](const BlockDesc &b) {
    const std::string &p = b.prefix;
    if (b.kind == 0) {
      add_param(m, p + ".normalize_1.weight", {b.cin});
      add_param(m, p + ".normalize_1.bias", {b.cin});
      add_param(m, p + ".conv_1.weight", {b.cout, b.cin, 3, 3, 3});
      add_param(m, p + ".conv_1.bias", {b.cout});
      add_param(m, p + ".dense_1.weight", {b.cout, tx});
      add_param(m, p + ".dense_1.bias", {b.cout});
      add_param(m, p + ".normalize_2.weight", {b.cout});
      add_param(m, p + ".normalize_2.bias", {b.cout});
      add_param(m, p + ".conv_2.weight", {b.cout, b.cout, 3, 3, 3});
      add_param(m, p + ".conv_2.bias", {b.cout});
      if (b.cin != b.cout) {
        add_param(m, p + ".match_input.weight", {b.cout, b.cin, 1, 1, 1});
        add_param(m, p + ".match_input.bias", {b.cout});
      }
      if (b.attention) {
        add_param(m, p + ".attention.group_norm.weight", {b.cout});
        add_param(m, p + ".attention.group_norm.bias", {b.cout});
        add_param(m, p + ".attention.mhsa.in_proj_weight", {3 * (int64_t)b.cout, b.cout});
        add_param(m, p + ".attention.mhsa.in_proj_bias", {3 * (int64_t)b.cout});
        add_param(m, p + ".attention.mhsa.out_proj.weight", {b.cout, b.cout});
        add_param(m, p + ".attention.mhsa.out_proj.bias", {b.cout});
      }
    } else if (b.kind == 1) {
      add_param(m, p + ".downsample.weight", {b.cout, b.cin, 3, 3, 3});
      add_param(m, p + ".downsample.bias", {b.cout});
    } else {
      add_param(m, p + ".upsample.1.weight", {b.cout, b.cin, 3, 3, 3});
      add_param(m, p + ".upsample.1.bias", {b.cout});
    }
  };
  for (auto &b : m->enc) add_block_params(b);
  for (auto &b : m->bott) add_block_params(b);
  for (auto &b : m->dec) add_block_params(b);
  add_param(m, "final.0.weight", {m->final_ch});
  add_param(m, "final.0.bias", {m->final_ch});
  add_param(m, "final.2.weight", {c.out_channels, m->final_ch, 3, 3, 3});
  add_param(m, "final.2.bias", {c.out_channels});
}

// A host-only handle (device < 0) can still build its op list (build_ops, resolve_conv) for the planners' self-tests: its "device"
// buffers are zeroed host memory that nothing launches on, and the few device calls of that path go through CM_DEV.
#define CM_DEV(m, expr) do { if ((m)->device >= 0) CM_HIP(expr); } while (0)

int dev_alloc(cm_model *m, void **p, size_t bytes) {
  if (m->device < 0) { if (!(*p = calloc(bytes ? bytes : 4, 1))) return fail("out of host memory"); }
  else CM_HIP(hipMalloc(p, bytes ? bytes : 4));
  m->allocs.push_back(*p);
  return 0;
}

int upload(cm_model *m, const std::vector<float> &h, float **d) {
  if (dev_alloc(m, (void **)d, h.size() * sizeof(float))) return 1;
  if (m->device < 0) std::memcpy(*d, h.data(), h.size() * sizeof(float));
  else CM_HIP(hipMemcpy(*d, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
  return 0;
}

Act *new_act(cm_model *m, const std::string &name, int C, int Z, int Y, int X, bool stats, int *rc) {
  auto a = std::make_unique<Act>();
  a->name = name;
  a->C = C; a->Z = Z; a->Y = Y; a->X = X;
  const size_t B = (size_t)m->cfg.max_batch;
  if (dev_alloc(m, (void **)&a->d, B * a->V() * C * sizeof(float))) { *rc = 1; return nullptr; }
  if (stats) {
    a->nslice = std::max(1, std::min(MAX_SLICES, a->V() / 128));
    if (dev_alloc(m, (void **)&a->part, B * MAX_SLOTS * C * 2 * sizeof(float))) { *rc = 1; return nullptr; }
    if (dev_alloc(m, (void **)&a->cnt, B * MAX_SLOTS * sizeof(float))) { *rc = 1; return nullptr; }
  }
  Act *r = a.get();
  m->acts.push_back(std::move(a));
  if (!name.empty()) m->act_by_name[name] = r;
  return r;
}

const Param &P(const cm_model *m, const std::string &name) { return m->params[m->pindex.at(name)]; }

// Weight fragments: every layout (generic MFMA order, parity fold of the upsample conv, Winograd, quarter resolution, first / last
// conv, attention) with its f16 / split flavours is defined once in cm_pack.h -- for the values packed here when a handle loads and
// for the index maps the device re-packs through after an optimizer step (cm_train_host.inc: train_setup).

int pick_ck(int C0, int C1) {
  for (int ck : {32, 16, 8})
    if (C0 % ck == 0 && C1 % ck == 0) return ck;
  return 0;
}

// Measured tile choices for the layer shapes of the reference configurations (tools/tune_tiles.py on
// one MI355X at B = 64, standalone launches): the analytic score below orders candidates well within a
// shape class but not across accumulator blockings.  Keyed by the layer shape only -- never by the batch --
// so the geometry, and with it every rounding, stays independent of how a batch is sharded.
struct TunedTile { int ntaps, stride, par, Ci, Co, Zo, Yo, Xo, NB, MB, bz, by, bx; };
const TunedTile kTunedTiles[] = {
#include "cm_tuned_tiles.inc"
    {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}};

const TunedTile *find_tuned(const cm::ConvArgs &a, int NB /* 0: any */) {
  static const bool off = cm::diag_env("CM_NO_TUNED") != nullptr;
  if (off) return nullptr;
  for (const TunedTile *t = kTunedTiles; t->ntaps; ++t)
    if (t->ntaps == a.ntaps && t->stride == a.stride && t->par == a.par && t->Ci == a.C0 + a.C1 && t->Co == a.Co &&
        t->Zo == a.Zo && t->Yo == a.Yo && t->Xo == a.Xo && (NB == 0 || t->NB == NB))
      return t;
  return nullptr;
}

// Tile geometry for one conv at batch B: choose the output box (bs,bz,by,bx) and
// the per-wave accumulator blocking MB (NB is fixed by the packed weights).
// Tile geometry is chosen for a fixed reference batch, never for the batch at hand: the
// fused GroupNorm statistics are summed per tile, so a geometry that changed with the
// batch size would make sample i of a shard differ in the last bits from sample i of the
// unsharded batch (SURVEY.md section 8e asks for bit-identical shards).
constexpr int TUNE_BATCH = 64;

// First conv (cm_conv_io.hip): tiles are bz x by planes of FULL x-rows; op.MB = 32-row blocks per tile
// (= statistics slots per tile).  Score: fill of the last block, balance over the 4 waves, halo overhead,
// enough tiles for the chip at the reference batch.
void pick_tile_first(Op &op) {
  cm::ConvArgs &a = op.ca;
  double best = -1;
  int bbz = 1, bby = 1;
  a.bs = 1; a.bx = a.Xo;
  for (int bz = 1; bz <= a.Zo; ++bz)
    for (int by = 1; by <= a.Yo; ++by) {
      if (a.Zo % bz || a.Yo % by) continue;
      a.bz = bz; a.by = by;
      const int nbox = bz * by * a.Xo, nblk = (nbox + 31) / 32;
      if (nblk > 16 || cm::conv_first_lds(a, op.first_cin) > 48 * 1024) continue;
      const double tiles = (double)(a.Zo / bz) * (a.Yo / by) * TUNE_BATCH;
      if ((a.Zo / bz) * (a.Yo / by) * nblk > MAX_SLOTS) continue;
      const double eff = (double)nbox / (32.0 * nblk);
      const double bal = (double)nblk / (4.0 * ((nblk + 3) / 4));
      const double halo = (double)nbox / ((bz + 2.0) * (by + 2.0) * (a.Xo + 2.0));
      const double score = eff * bal * (0.5 + 0.5 * halo) * std::min(1.0, tiles / 512.0);
      if (score > best) { best = score; bbz = bz; bby = by; }
    }
  a.bz = bbz; a.by = bby;
  a.ntz = a.Zo / bbz; a.nty = a.Yo / bby; a.ntx = 1;
  op.MB = cm::conv_first_blocks(a);
}

void pick_tile(Op &op, int B) {
  cm::ConvArgs &a = op.ca;
  const int NB = op.NB;
  static const int force_mb = cm::diag_env("CM_FORCE_MB") ? atoi(cm::diag_env("CM_FORCE_MB")) : 0;
  const int osd = a.par ? 2 : 1;  // parity mode tiles the low-resolution source grid
  const int Zo = a.Zo / osd, Yo = a.Yo / osd, Xo = a.Xo / osd;
  const int vox = Zo * Yo * Xo;
  // largest accumulator blocking that still fits 256 VGPRs (2 waves/SIMD) without spilling;
  // the register-ring fast path (CK == 32) carries more live state than the generic one
  const bool fastp = a.CK == 32 && (a.ntaps == 27 || a.ntaps == 8);
  const int max_blk = fastp ? ((NB == 1) ? 5 : (NB == 2 ? 2 : 1)) : ((NB == 1) ? 8 : (NB == 2 ? 4 : 2));
  if (const TunedTile *t = find_tuned(a, NB)) {
    const int osdt = a.par ? 2 : 1;
    a.bs = 1; a.bz = t->bz; a.by = t->by; a.bx = t->bx;
    if (cm::conv_variant_exists(t->MB, NB) && (t->bz * t->by * t->bx + 31) / 32 == t->MB && cm::conv_lds_bytes(a, t->MB, NB) <= 80 * 1024 &&
        (!op.small_n || !(t->MB & (t->MB - 1)))) {
      op.MB = t->MB;
      a.ntz = (a.Zo / osdt + a.bz - 1) / a.bz; a.nty = (a.Yo / osdt + a.by - 1) / a.by; a.ntx = (a.Xo / osdt + a.bx - 1) / a.bx;
      return;
    }
  }
  double best = -1;
  int bbs = 1, bbz = 1, bby = 1, bbx = 1, bMB = 1;
  const int ntn = (a.Co + 32 * NB - 1) / (32 * NB);
  const int max_bs = (vox <= 64 && !op.stat_act && !op.small_n) ? 4 : 1;  // fused statistics need one sample per tile
  for (int bs = 1; bs <= max_bs; ++bs)
    for (int bz = 1; bz <= Zo; ++bz)
      for (int by = 1; by <= Yo; ++by)
        for (int bx = 1; bx <= Xo; ++bx) {
          const int nbox = bs * bz * by * bx;
          const int MB = (nbox + 31) / 32;
          if (MB > max_blk) continue;
          if (op.small_n && (MB & (MB - 1))) continue;  // its thread groups need 256 % (32 MB) == 0
          if (force_mb && MB != force_mb && vox >= 128) continue;
          a.bs = bs; a.bz = bz; a.by = by; a.bx = bx;
          const size_t lds = cm::conv_lds_bytes(a, MB, NB);
          if (lds > 64 * 1024) continue;
          const long ntz = (Zo + bz - 1) / bz, nty = (Yo + by - 1) / by, ntx = (Xo + bx - 1) / bx, nts = (B + bs - 1) / bs;
          const double tiles = (double)ntz * nty * ntx * nts * ntn * (a.par ? 8 : 1);
          const double util = (double)vox * B * ntn / (tiles * 32.0 * MB);
          // work per tile in accumulator blocks; balance over 256 CUs
          const double per_cu = std::ceil(tiles / 256.0);
          const double balance = tiles / (per_cu * 256.0);
          // halo overhead (staging) and register-occupancy preference
          const double hv = (double)bs * ((bz - 1) * a.stride + a.td) * ((by - 1) * a.stride + a.td) *
                            ((bx - 1) * a.stride + a.td);
          const double halo = 1.0 / (1.0 + 0.02 * hv / (32.0 * MB));
          const double occ = (MB * NB <= 4) ? 1.0 : 0.93;
          const double amort = 1.0 - 0.06 / (MB * NB);  // larger blocks amortise loads/epilogue
          const double score = util * std::min(1.0, 0.25 + balance) * halo * occ * amort;
          if (score > best) { best = score; bbs = bs; bbz = bz; bby = by; bbx = bx; bMB = MB; }
        }
  a.bs = bbs; a.bz = bbz; a.by = bby; a.bx = bbx;
  op.MB = bMB;
  a.ntz = (Zo + bbz - 1) / bbz; a.nty = (Yo + bby - 1) / bby; a.ntx = (Xo + bbx - 1) / bbx;
}

struct ConvSpec {
  const Act *s0;
  const Act *s1 = nullptr;
  const float *gn = nullptr;
  int silu = 0;
  std::string wname, bname;
  int ntaps = 27, stride = 1, ups = 0;
  const float *temb = nullptr;
  const Act *resid = nullptr;
  Act *out = nullptr;
  int Co = 0;
  int ci_valid = -1;  // valid input channels of the reference weight (first conv: 3 of 8)
  bool stats = false; // produce the GroupNorm statistics of `out` in the epilogue
  int pm_off = -1;    // Dropout3d mask slice of the input (conv_2 of a ResnetBlock)
  const Act *skip0 = nullptr, *skip1 = nullptr;  // block input whose match_input conv may be fused in
  std::string skip_w, skip_b;
};

// ---- "h2" arithmetic (cm_kernels.h: cm_split2_f16): operand range management ---------------------------------------------------
// f16 has 5 exponent bits.  Weights: packed as w * 2^k (cm_pack.h: h2_wscale); the kernel multiplies its fp32 accumulators by 2^-k
// (exact).  Activations: a GroupNorm output
// satisfies |z| < sqrt(n) for a group of n elements, so |SiLU(gamma z + beta)| <= sqrt(n) max|gamma| + max|beta|, times `gain` for a
// linear input transform (4 for the Winograd B^T d B: sums of four values).  A layer whose bound exceeds 32000 keeps the six-term
// bf16 form (bf16 has the exponent range of fp32).
static bool h2_bound_ok(const std::vector<float> &g, const std::vector<float> &b, const Op &gop, double gain);
static bool h2_act_bounded(const cm_model *m, const Op &gop, double gain) {
  return h2_bound_ok(P(m, gop.gname).host, P(m, gop.bename).host, gop, gain);
}
static bool h2_bound_ok(const std::vector<float> &g, const std::vector<float> &b, const Op &gop, double gain) {
  double gm = 0, bm = 0;
  for (float v : g) gm = std::max(gm, (double)std::fabs(v));
  for (float v : b) bm = std::max(bm, (double)std::fabs(v));
  const int Ct = gop.g0->C + (gop.g1 ? gop.g1->C : 0);
  const double n = (double)(Ct / GN_GROUPS) * gop.g0->V();
  const double bound = (std::sqrt(n) * gm + bm) * gain;
  return std::isfinite(bound) && bound <= 32000.0;
}

// h2 fragments and weight scale 2^k (0: none) of a conv op from its weight in the REFERENCE layout (cm_pack.h: h2_fragments); add_conv
// uploads them at load time, refresh_h2 copies them over the same buffer after training.  Every h2 layer has Ci_ref == Ci_pad.
static float h2_pack(const Op &op, H2Kind kind, const float *w_ref, std::vector<float> *frag) {
  return h2_fragments(kind, w_ref, op.ca.Co, op.ca.C0 + op.ca.C1, frag);
}
// load time: the op takes the h2 form `kind` if its weights have a scale (H2_FIN: packed on the device from d_wfin_src)
static int add_h2(cm_model *m, Op &op, H2Kind kind, const float *w_ref, float **d_frag) {
  std::vector<float> frag;
  const float ws = h2_pack(op, kind, w_ref, &frag);
  if (!(ws > 0.f)) return 0;
  if (kind == H2_FIN) {
    if (dev_alloc(m, (void **)d_frag, cm::CM_FIN_W_FLOATS * sizeof(float))) return 1;
    CM_DEV(m, cm::launch_fin_pack(op.d_wfin_src, *d_frag, op.ca.Co, 2, m->stream, ws));
    CM_DEV(m, hipStreamSynchronize(m->stream));
  } else if (upload(m, frag, d_frag)) return 1;
  op.h2_oscale = 1.f / ws;
  return 0;
}

// h2 fragments of an attention block's two weights (reference layout [3E][E], [E][E]); *osc_* = 2^-k of each, 0 where the weight has no
// scale (all-zero or non-finite: the fragments are zeros and the plan keeps the two-launch path)
static void attn_pack_h2(const float *w_in, const float *w_out, int E, std::vector<float> *f_in, std::vector<float> *f_out, float *osc_in,
                         float *osc_out) {
  const float wsi = h2_wscale(w_in, (size_t)3 * E * E), wso = h2_wscale(w_out, (size_t)E * E);
  *f_in = pack_attn_h2(w_in, 3 * E, E, wsi);
  *f_out = pack_attn_h2(w_out, E, E, wso);
  *osc_in = wsi > 0.f ? 1.f / wsi : 0.f;
  *osc_out = wso > 0.f ? 1.f / wso : 0.f;
}

int add_conv(cm_model *m, const ConvSpec &s) {
  Op op;
  op.kind = OP_CONV;
  op.cls = s.ntaps == 27 ? K_CONV3 : K_CONV1;
  cm::ConvArgs &a = op.ca;
  a.src0 = s.s0->d; a.C0 = s.s0->C;
  a.src1 = s.s1 ? s.s1->d : nullptr; a.C1 = s.s1 ? s.s1->C : 0;
  a.gn = s.gn; a.silu = s.silu;
  a.Zs = s.s0->Z; a.Ys = s.s0->Y; a.Xs = s.s0->X;
  a.Zo = s.out->Z; a.Yo = s.out->Y; a.Xo = s.out->X;
  a.ntaps = s.ntaps; a.stride = s.stride; a.ups = s.ups;
  a.td = s.ntaps == 27 ? 3 : 1; a.par = 0; a.wpar_stride = 0;
  const bool parity = s.ups && s.ntaps == 27 && !cm::diag_env("CM_NO_PARITY_UPCONV");
  if (parity) { a.ups = 0; a.par = 1; a.td = 2; a.ntaps = 8; }
  a.out = s.out->d; a.out_cs = s.out->C; a.Co = s.Co;
  a.temb = s.temb; a.temb_stride = m->nproj; a.tidx = m->tbuf;
  a.resid = s.resid ? s.resid->d : nullptr; a.res_cs = s.resid ? s.resid->C : 0;
  a.CK = pick_ck(a.C0, a.C1);
  if (s.ntaps == 1) {
    // 1x1x1 convs have no halo: stage as many channels per pass as the sources allow
    // (a chunk may not straddle the concat boundary), so a whole K = Ci contraction needs
    // one or two staging rounds instead of Ci/32.
    for (int ck : {256, 128, 64})
      if (a.C0 % ck == 0 && a.C1 % ck == 0) { a.CK = ck; break; }
  }
  if (!a.CK) return fail("conv %s: channel counts %d/%d not multiples of 8", s.wname.c_str(), a.C0, a.C1);
  a.nch0 = a.C0 / a.CK; a.nch1 = a.C1 / a.CK;
  op.NB = s.Co > 32 ? 2 : 1;
  // full- and half-resolution stride-1 3x3x3 layers: Winograd F(2x2,3x3) over (Y, X) -- 2.25x fewer matrix
  // instructions (cm_conv_wino.hip); its workgroups own one 32-channel output tile each
  {
    int wz = 0, wy = 0, wx = 0;
    op.wino = s.ntaps == 27 && s.stride == 1 && !s.ups && a.C0 % 16 == 0 && a.C1 % 16 == 0 && s.Co % 32 == 0 && s.Co == s.out->C &&
              s.ci_valid < 0 && s.out->V() > 64 && cm::conv_wino_pick(s.out->Z, s.out->Y, s.out->X, &wz, &wy, &wx) && !cm::diag_env("CM_NO_WINO");
  }
  // tiny-spatial layers keep NB = 2: NB = 4 tiles (all 128 output channels per workgroup) spill ~80 VGPRs on the register-ring
  // path and measured no better than two NB = 2 workgroups
  if (s.ntaps == 27 && s.out->V() <= 64 && cm::diag_env("CM_QR_NB")) op.NB = atoi(cm::diag_env("CM_QR_NB"));
  if (op.wino) op.NB = 1;
  if (s.ntaps == 27 && s.out->V() > 64 && !op.wino) {
    if (const TunedTile *t = find_tuned(a, 0)) op.NB = t->NB;
    // tuner policies (tools/tune_tiles.py): N blocking of the 64- / 128-channel 3x3x3 layers
    if (s.Co == 64 && cm::diag_env("CM_NB64")) op.NB = atoi(cm::diag_env("CM_NB64"));
    if (s.Co == 128 && cm::diag_env("CM_NB128")) op.NB = atoi(cm::diag_env("CM_NB128"));
  }
  const Param &w = P(m, s.wname);
  const Param &b = P(m, s.bname);
  const int Ci_ref = (int)w.shape[1];
  const int Ci_pad = a.C0 + a.C1;
  if (Ci_ref > Ci_pad || (s.ci_valid < 0 && Ci_ref != Ci_pad))
    return fail("conv %s: weight has %d input channels, sources provide %d", s.wname.c_str(), Ci_ref, Ci_pad);
  const int Co_ref = (int)w.shape[0];
  const std::vector<float> wi = to_internal_taps(w.host.data(), Co_ref, Ci_ref, s.ntaps);
  const std::vector<float> wp = parity ? parity_weights(wi, Co_ref, Ci_ref) : std::vector<float>();   // [8 classes][Co][Ci][8]
  std::vector<float> wf;
  if (parity) {
    wf = pack_parity_classes(wp, &a.wpar_stride, [&](const float *w8) { return pack_conv(w8, Co_ref, Ci_ref, 8, Ci_pad, a.CK, op.NB); });
    if (m->precision == CM_PRECISION_F16 && a.CK == 32) {   // reduced-precision plan: the same fragments as f16
      const std::vector<float> wf16 =
          pack_parity_classes(wp, &op.wpar_stride16, [&](const float *w8) { return pack_conv_f16(w8, Co_ref, Ci_ref, 8, Ci_pad, a.CK, op.NB); });
      if (upload(m, wf16, &op.d_wfrag16)) return 1;
    }
  } else {
    wf = pack_conv(wi.data(), Co_ref, Ci_ref, s.ntaps, Ci_pad, a.CK, op.NB);
    // reduced-precision plan: 1x1x1 convs without output statistics (attention in-projection, unfused skip convs) on f16 operands
    if (m->precision == CM_PRECISION_F16 && s.ntaps == 1 && s.stride == 1 && !s.ups && !s.stats && !s.temb && Ci_ref == Ci_pad &&
        a.C0 % 16 == 0 && a.C1 % 16 == 0 && !cm::diag_env("CM_NO_1X1_F16") &&
        upload(m, pack_1x1_f16(wi.data(), Co_ref, Ci_ref, op.NB), &op.d_w1x1_16))
      return 1;
  }
  // upsample convs: the source tile staged once for four parity classes (cm_conv_ups.hip) when a tile fits
  if (parity && a.CK == 32 && !s.s1 && !s.gn && !s.temb && !s.resid && s.Co % 32 == 0 && s.Co == s.out->C && !cm::diag_env("CM_NO_UPS") &&
      cm::conv_ups_pick(a.Zs, a.Ys, a.Xs, &op.ups_tz, &op.ups_ty, &op.ups_tx, &op.ups_mbw, &op.ups_planes) &&
      (a.Zs / op.ups_tz) * (a.Ys / op.ups_ty) * (a.Xs / op.ups_tx) * 8 * op.ups_mbw <= MAX_SLOTS)   // (its statistics slots must fit)
    op.ups = true;
  if (op.ups && m->precision != CM_PRECISION_F16 && Ci_ref == Ci_pad && Ci_ref % 32 == 0 && !cm::diag_env("CM_NO_UPS_B6")) {
    const std::vector<float> wb6 = pack_parity_classes(wp, &op.wups_b6_stride, [&](const float *w8) { return pack_ups_b6(w8, Co_ref, Ci_ref); });
    if (upload(m, wb6, &op.d_wups_b6)) return 1;
    // default plan: h2 with a per-sample scale taken from the source tensor's slot statistics (cm_conv_ups.hip, PREC = 4) -- the
    // source is a block output with statistics (every conv_2 / attention output carries them)
    if (m->precision == CM_PRECISION_F32 && !cm::diag_env("CM_NO_H2") && !cm::diag_env("CM_NO_UPS_H2") && s.s0->part &&
        add_h2(m, op, H2_UPS, w.host.data(), &op.d_wups_h2))
      return 1;
  }
  if (op.ups && m->precision == CM_PRECISION_F16 && Ci_ref == Ci_pad && Ci_ref % 32 == 0 && !cm::diag_env("CM_NO_UPS_F16")) {
    const std::vector<float> w16 = pack_parity_classes(wp, &op.wups16_stride, [&](const float *w8) { return pack_ups_f16(w8, Co_ref, Ci_ref); });
    if (upload(m, w16, &op.d_wups16)) return 1;
  }
  // the UNet's last conv (base -> C channels): vector-ALU kernel instead of a 32-wide MFMA tile
  if (s.ntaps == 27 && s.stride == 1 && !s.ups && s.Co <= 8 && !s.stats && !s.temb && !s.resid &&
      !cm::diag_env("CM_NO_SMALLN")) {
    op.small_n = true;
    op.small_nco = s.Co <= 4 ? 4 : 8;
    if (upload(m, pack_small(wi.data(), s.Co, Ci_ref, Ci_pad, a.CK, op.small_nco), &op.d_wsmall)) return 1;
    // the same layer on the matrix core (round 4): 27 taps x 4 channels = 108 columns of a GEMM over the 32 input channels
    if (s.Co <= 4 && Ci_ref == 32 && Ci_pad == 32 && !s.s1 && !cm::diag_env("CM_NO_FIN") && cm::conv_fin_pick(s.out->Y, s.out->X, &op.fin_by, &op.fin_bx)) {
      if (upload(m, w.host, &op.d_wfin_src)) return 1;
      if (dev_alloc(m, (void **)&op.d_wfin, cm::CM_FIN_W_FLOATS * sizeof(float))) return 1;
      CM_DEV(m, cm::launch_fin_pack(op.d_wfin_src, op.d_wfin, s.Co, 0, m->stream));
      if (m->precision == CM_PRECISION_F16) {
        if (dev_alloc(m, (void **)&op.d_wfin16, cm::CM_FIN_W_FLOATS * sizeof(float))) return 1;
        CM_DEV(m, cm::launch_fin_pack(op.d_wfin_src, op.d_wfin16, s.Co, 1, m->stream));
      }
      CM_DEV(m, hipStreamSynchronize(m->stream));
      op.fin = true;
    }
  }
  if (op.wino) {
    const std::vector<float> ww = pack_wino(wi, s.Co, Ci_ref, Ci_pad);
    if (upload(m, ww, &op.d_wwino)) return 1;
    if (m->precision == CM_PRECISION_F16 && upload(m, pack_wino_f16(wi, s.Co, Ci_ref, Ci_pad), &op.d_wwino16)) return 1;
    op.wwino_floats = (long long)ww.size();
    {
      int wz = 0, wy = 0, wx = 0;
      if (m->precision != CM_PRECISION_F16 && !cm::diag_env("CM_NO_WINO_B6") && cm::conv_wino_pick(s.out->Z, s.out->Y, s.out->X, &wz, &wy, &wx) &&
          cm::conv_wino_b6_ok(wz, wy, wx, s.Co, s.out->Z) && upload(m, pack_wino_b6(ww), &op.d_wwino_b6))
        return 1;
    }
    // reduced-precision plan: the direct f16 kernel replaces the Winograd one where its tiles fit (no transforms to pay for
    // when the matrix instruction is 16x faster)
    // (measured on the 24x72 grid, B = 32: 61 vs 70 us on the 32 -> 32 full-resolution layer, 136 vs 154 us on 96 -> 32, 72 vs 76 us
    // at half resolution; on two-plane grids the two-tile Winograd form stays: 24 vs 47 us)
    if (m->precision == CM_PRECISION_F16 && Ci_ref == Ci_pad && a.C0 % 16 == 0 && a.C1 % 16 == 0 && s.out->Z >= 4 && !cm::diag_env("CM_NO_F16D") &&
        cm::conv_f16d_pick(s.out->Z, s.out->Y, s.out->X, &op.f16d_bz, &op.f16d_by, &op.f16d_bx, &op.f16d_mbw)) {
      if (upload(m, pack_f16d(wi.data(), s.Co, Ci_ref, 27, s.Co % 64 == 0 ? 2 : 1), &op.d_w16d)) return 1;
      op.f16d = true;
    }
  }
  // the UNet's first conv (C <= 8 data channels -> base): dedicated kernel, whole weight set in registers
  if (s.s0 == m->x8_act && s.ntaps == 27 && s.stride == 1 && !s.ups && !s.gn && !s.temb && !s.resid && !s.s1 &&
      s.Co % 32 == 0 && Ci_ref <= 8 && !cm::diag_env("CM_NO_FIRSTK")) {
    op.first_k = true;
    op.first_cin = Ci_ref <= 4 ? 4 : 8;
    if (upload(m, pack_first(wi.data(), s.Co, Ci_ref, op.first_cin), &op.d_wfirst)) return 1;
  }
  float *dw = nullptr, *db = nullptr;
  if (upload(m, wf, &dw)) return 1;
  const int TN = 32 * op.NB, co_pad = (s.Co + TN - 1) / TN * TN;
  std::vector<float> bp((size_t)co_pad, 0.f);
  std::copy(b.host.begin(), b.host.end(), bp.begin());
  if (upload(m, bp, &db)) return 1;
  a.wfrag = dw; a.bias = db;
  if (s.stats && !cm::diag_env("CM_NO_FUSED_STATS")) op.stat_act = s.out;
  op.out_act = s.out;
  op.resid_act = s.resid;
  op.pm_off = s.pm_off;
  op.in0 = s.s0; op.in1 = s.s1;
  op.wname = s.wname; op.bname = s.bname;
  op.ref_taps = s.ntaps;
  op.temb_off = s.temb ? (int)(s.temb - m->temb_table) : -1;
  if (s.gn)
    for (int i = (int)m->ops.size() - 1; i >= 0; --i)
      if (m->ops[i].kind == OP_GNFIN && m->ops[i].gn_out == s.gn) { op.gn_op = i; break; }
  const bool h2_plan = m->precision == CM_PRECISION_F32 && !cm::diag_env("CM_NO_H2") && s.gn && op.gn_op >= 0 && s.silu;
  if (op.fin && h2_plan && h2_act_bounded(m, m->ops[op.gn_op], 1.0) && add_h2(m, op, H2_FIN, w.host.data(), &op.d_wfin_h2)) return 1;
  if (op.wino && op.d_wwino_b6 && h2_plan && h2_act_bounded(m, m->ops[op.gn_op], 4.0) && add_h2(m, op, H2_WINO, w.host.data(), &op.d_wwino_h2))
    return 1;
  // Tiny-spatial layers (one 54-voxel tile per sample at quarter resolution): the only way to
  // more parallelism AND less weight traffic per workgroup is to split K over workgroups;
  // a second pass sums the partials in a fixed order and applies the epilogue.
  const int nchunks = a.nch0 + a.nch1;
  static const int qr_vmax = cm::diag_env("CM_QR_VMAX") ? atoi(cm::diag_env("CM_QR_VMAX")) : 96;   // HERMES-CR-120 quarter resolution: 84 voxels
  if (s.ntaps == 27 && !parity && a.CK == 32 && nchunks >= 2 && s.out->V() <= qr_vmax && s.Co <= 256 && s.Co == s.out->C &&
      op.stat_act && !cm::diag_env("CM_NO_KSPLIT")) {
    static const int qr_ks = cm::diag_env("CM_QR_KS") ? atoi(cm::diag_env("CM_QR_KS")) : 4;
    op.ks = std::max(1, std::min(nchunks, s.out->V() > 64 ? std::min(qr_ks, 2) : qr_ks));   // (84 voxels: ks 2 3.06 ms, ks 4 3.12, none 3.16 per CR-120 step)
    const size_t need = (size_t)op.ks * m->cfg.max_batch * s.out->V() * s.Co;
    m->ks_scratch_floats = std::max(m->ks_scratch_floats, need);
    std::vector<float> zb((size_t)co_pad, 0.f);
    if (upload(m, zb, &op.d_zero_bias)) return 1;
  }
  // fuse the 1x1x1 skip conv when this conv runs on the 27-tap register-ring path without K split
  if (s.skip0 && s.ntaps == 27 && !parity && a.CK == 32 && !op.small_n && (!op.wino || op.NB == 1) && s.stride == 1 &&
      s.skip0->C % 32 == 0 && (!s.skip1 || s.skip1->C % 32 == 0) && !cm::diag_env("CM_NO_FUSE_SKIP")) {
    const Param &w2 = P(m, s.skip_w);
    const Param &b2 = P(m, s.skip_b);
    const int Ci2 = (int)w2.shape[1];
    if (Ci2 == s.skip0->C + (s.skip1 ? s.skip1->C : 0) && (int)w2.shape[0] == s.Co) {
      std::vector<float> w2f = pack_conv(w2.host.data(), s.Co, Ci2, 1, Ci2, 32, op.NB);
      if (upload(m, w2f, &op.d_s2w)) return 1;
      std::vector<float> bf((size_t)co_pad, 0.f);
      for (int i = 0; i < s.Co; ++i) bf[i] = b.host[i] + b2.host[i];
      if (upload(m, bf, &op.d_bias_fused)) return 1;
      op.skip0 = s.skip0; op.skip1 = s.skip1; op.skip_w = s.skip_w; op.skip_b = s.skip_b;
    }
  }
  if (op.f16d && op.d_s2w) {
    const Param &w2 = P(m, s.skip_w);
    const int Cs = (int)w2.shape[1];
    if (Cs % 16 == 0 && s.skip0->C % 16 == 0 && (!s.skip1 || s.skip1->C % 16 == 0)) {
      if (upload(m, pack_f16d(w2.host.data(), s.Co, Cs, 1, s.Co % 64 == 0 ? 2 : 1), &op.d_w16d_skip)) return 1;
    } else {
      op.f16d = false;
    }
  }
  // Lowest resolution (two z planes, <= 64 voxels per plane): whole-sample kernel with the GroupNorm finalisation of its
  // input inside (cm_conv_qr.hip), inference plan.  The K-split / generic set-up above stays for the training forward.
  if (s.ntaps == 27 && !parity && s.stride == 1 && !s.ups && s.gn && op.gn_op >= 0 && s.ci_valid < 0 && s.out->Z == 2 && s.s0->Z == 2 &&
      s.out->Y * s.out->X <= 64 && s.Co % 32 == 0 && s.Co == s.out->C && op.stat_act && (!s.skip0 || op.d_s2w) &&
      !cm::diag_env("CM_NO_QR")) {
    cm::QrArgs q{};
    q.C0 = a.C0; q.C1 = a.C1; q.Co = s.Co; q.Y = s.out->Y; q.X = s.out->X; q.groups = GN_GROUPS; q.gamma = m->ops[op.gn_op].gamma;
    if (op.d_s2w) { q.s2w = op.d_s2w; q.s2C0 = s.skip0->C; q.s2C1 = s.skip1 ? s.skip1->C : 0; }
    if (cm::conv_qr_ok(q)) {
      {
        const std::vector<float> wq = pack_qr(wi, s.Co, Ci_ref);
        if (upload(m, wq, &op.d_wqr)) return 1;
        op.wqr_floats = (long long)wq.size();
        if (m->precision != CM_PRECISION_F16 && Ci_ref % 64 == 0 && !cm::diag_env("CM_NO_QR_B6") && upload(m, pack_qr_b6(wq, s.Co, Ci_ref), &op.d_wqr_b6))
          return 1;
        if (op.d_wqr_b6 && h2_plan && h2_act_bounded(m, m->ops[op.gn_op], 1.0) && add_h2(m, op, H2_QR, w.host.data(), &op.d_wqr_h2)) return 1;
      }
      if (op.d_s2w) {
        const Param &w2 = P(m, s.skip_w);
        if (upload(m, pack_qr_skip(w2.host.data(), s.Co, (int)w2.shape[1]), &op.d_wqr_skip)) return 1;
      }
      op.qr = true;
      m->ops[op.gn_op].qr_consumer = true;
    }
  }
  op.flops_per_sample = 2.0 * s.out->V() * s.Co * (double)Ci_ref * s.ntaps;
  op.label = s.wname;
  m->ops.push_back(op);
  return 0;
}

void add_stats(cm_model *m, const Act *a) {
  if (!cm::diag_env("CM_NO_FUSED_STATS")) return;  // the producing conv writes the statistics in its epilogue
  Op op;
  op.kind = OP_STATS; op.cls = K_NORM; op.act = a; op.label = "stats(" + a->name + ")";
  m->ops.push_back(op);
}

int add_gnfin(cm_model *m, const Act *g0, const Act *g1, const std::string &wname, const std::string &bname, float **gn_out) {
  Op op;
  op.kind = OP_GNFIN; op.cls = K_NORM; op.g0 = g0; op.g1 = g1; op.label = "gn_finalize(" + wname + ")";
  op.gname = wname; op.bename = bname;
  float *dg = nullptr, *db = nullptr;
  if (upload(m, P(m, wname).host, &dg)) return 1;
  if (upload(m, P(m, bname).host, &db)) return 1;
  op.gamma = dg; op.beta = db;
  const int Ct = g0->C + (g1 ? g1->C : 0);
  if (dev_alloc(m, (void **)&op.gn_out, (size_t)m->cfg.max_batch * 2 * Ct * sizeof(float))) return 1;
  *gn_out = op.gn_out;
  m->ops.push_back(op);
  return 0;
}

int build_ops(cm_model *m) {
  const cm_unet_config &c = m->cfg;
  const int L = m->L();
  int rc = 0;
  // spatial dims per level: conv k3 s2 p1 -> floor((n-1)/2)+1  (layers.py:84)
  std::vector<int> Zl{L}, Yl{c.rows}, Xl{c.cols};
  for (int l = 1; l < c.n_levels; ++l) {
    Zl.push_back((Zl.back() - 1) / 2 + 1);
    Yl.push_back((Yl.back() - 1) / 2 + 1);
    Xl.push_back((Xl.back() - 1) / 2 + 1);
  }
  for (int l = 1; l < c.n_levels; ++l)
    if (Zl[l] * 2 != Zl[l - 1] || Yl[l] * 2 != Yl[l - 1] || Xl[l] * 2 != Xl[l - 1])
      return fail("grid %dx%dx%d is not divisible by 2^%d: the reference's skip concat (unet.py:160) would fail too",
                  c.rows, c.cols, L, c.n_levels - 1);

  // time-embedding projection table offsets (one slice of nproj per res block)
  std::map<std::string, int> temb_off;
  {
    int off = 0;
    auto visit = [&](const BlockDesc &b) { if (b.kind == 0) { temb_off[b.prefix] = off; off += b.cout; } };
    for (auto &b : m->enc) visit(b);
    for (auto &b : m->bott) visit(b);
    for (auto &b : m->dec) visit(b);
    m->nproj = off;
  }
  if (dev_alloc(m, (void **)&m->temb_table, (size_t)TIME_ROWS * m->nproj * sizeof(float))) return 1;

  // input / output tensors
  auto xin = std::make_unique<Act>();
  xin->name = "input"; xin->C = 8; xin->Z = L; xin->Y = c.rows; xin->X = c.cols;
  if (dev_alloc(m, (void **)&xin->d, (size_t)c.max_batch * xin->V() * 8 * sizeof(float))) return 1;
  CM_DEV(m, hipMemset(xin->d, 0, (size_t)c.max_batch * xin->V() * 8 * sizeof(float)));
  m->x8 = xin->d; m->x8_act = xin.get();
  m->acts.push_back(std::move(xin));

  auto res_block = [&](const BlockDesc &b, const Act *x0, const Act *x1, Act **result) -> int {
    const int l = b.level;
    const std::string &p = b.prefix;
    float *gn1 = nullptr, *gn2 = nullptr;
    if (add_gnfin(m, x0, x1, p + ".normalize_1.weight", p + ".normalize_1.bias", &gn1)) return 1;
    Act *h1 = new_act(m, p + ".conv_1", b.cout, Zl[l], Yl[l], Xl[l], true, &rc);
    if (rc) return 1;
    ConvSpec c1; c1.s0 = x0; c1.s1 = x1; c1.gn = gn1; c1.silu = 1; c1.wname = p + ".conv_1.weight"; c1.bname = p + ".conv_1.bias";
    c1.temb = m->temb_table + temb_off[p]; c1.out = h1; c1.Co = b.cout; c1.stats = true;
    if (add_conv(m, c1)) return 1;
    add_stats(m, h1);
    if (add_gnfin(m, h1, nullptr, p + ".normalize_2.weight", p + ".normalize_2.bias", &gn2)) return 1;
    const Act *resid = x0;
    int mi_index = -1;
    if (b.cin != b.cout) {
      Act *r = new_act(m, p + ".match_input", b.cout, Zl[l], Yl[l], Xl[l], false, &rc);
      if (rc) return 1;
      ConvSpec cs; cs.s0 = x0; cs.s1 = x1; cs.ntaps = 1; cs.wname = p + ".match_input.weight"; cs.bname = p + ".match_input.bias";
      cs.out = r; cs.Co = b.cout;
      if (add_conv(m, cs)) return 1;
      mi_index = (int)m->ops.size() - 1;
      resid = r;
    } else if (x1) {
      return fail("identity skip with concatenated input is not expressible (block %s)", p.c_str());
    }
    Act *h2 = new_act(m, b.attention ? p + ".conv_2+skip" : p, b.cout, Zl[l], Yl[l], Xl[l], true, &rc);
    if (rc) return 1;
    ConvSpec c2; c2.s0 = h1; c2.gn = gn2; c2.silu = 1; c2.wname = p + ".conv_2.weight"; c2.bname = p + ".conv_2.bias";
    c2.resid = resid; c2.out = h2; c2.Co = b.cout; c2.stats = true; c2.pm_off = temb_off[p];
    if (mi_index >= 0) { c2.skip0 = x0; c2.skip1 = x1; c2.skip_w = p + ".match_input.weight"; c2.skip_b = p + ".match_input.bias"; }
    if (add_conv(m, c2)) return 1;
    if (mi_index >= 0 && m->ops.back().d_s2w) m->ops[mi_index].skip_if_fused = true;
    add_stats(m, h2);
    *result = h2;
    if (b.attention) {
      const std::string ap = p + ".attention";
      float *gna = nullptr;
      if (add_gnfin(m, h2, nullptr, ap + ".group_norm.weight", ap + ".group_norm.bias", &gna)) return 1;
      Act *qkv = new_act(m, ap + ".qkv", 3 * b.cout, Zl[l], Yl[l], Xl[l], false, &rc);
      if (rc) return 1;
      ConvSpec cq; cq.s0 = h2; cq.gn = gna; cq.silu = 0; cq.ntaps = 1; cq.wname = ap + ".mhsa.in_proj_weight"; cq.bname = ap + ".mhsa.in_proj_bias";
      cq.out = qkv; cq.Co = 3 * b.cout;
      if (add_conv(m, cq)) return 1;
      Act *ao = new_act(m, ap + ".core", b.cout, Zl[l], Yl[l], Xl[l], false, &rc);
      if (rc) return 1;
      Op at; at.kind = OP_ATTN; at.cls = K_ATTN; at.label = ap + ".core"; at.qkv = qkv->d; at.aout = ao->d; at.S = qkv->V(); at.E = b.cout;
      if ((size_t)2 * at.S * (at.E / ATTN_HEADS) * 4 > 160 * 1024)
        return fail("attention with %d tokens exceeds the LDS-resident K/V design", at.S);
      if (!cm::attn_core_width_ok(at.E, ATTN_HEADS))   // (no kernel, fused or not, takes it: said here, not by the first forward's launch)
        return fail("%s: %d channels over %d heads: head width outside the attention kernels' 8, 16, 32 and 64 channels per head", ap.c_str(), at.E, ATTN_HEADS);
      m->ops.push_back(at);
      Act *h3 = new_act(m, p, b.cout, Zl[l], Yl[l], Xl[l], true, &rc);
      if (rc) return 1;
      ConvSpec co; co.s0 = ao; co.ntaps = 1; co.wname = ap + ".mhsa.out_proj.weight"; co.bname = ap + ".mhsa.out_proj.bias";
      co.resid = h2; co.out = h3; co.Co = b.cout; co.stats = true;
      if (add_conv(m, co)) return 1;
      add_stats(m, h3);
      *result = h3;
      // Inference plan: the whole AttentionBlock as one launch per (head, sample) + the head combine
      // (cm_attn_block.hip) when the sample's tokens fit the LDS-resident design; the four generic ops above
      // stay in the list for the training forward (their activations feed the backward pass) and as fallback.
      const int nops = (int)m->ops.size();
      if (cm::attn_block_ok(qkv->V(), b.cout, ATTN_HEADS, GN_GROUPS) && !cm::diag_env("CM_NO_FUSED_ATTN") && !cm::diag_env("CM_NO_FUSED_STATS")) {
        Op fb;
        fb.kind = OP_ATTNBLK; fb.cls = K_ATTN; fb.label = ap + " (fused block)";
        fb.ab_x = h2; fb.ab_out = h3; fb.S = qkv->V(); fb.E = b.cout;
        fb.ab_gn = nops - 4; fb.ab_qkv = nops - 3; fb.ab_outc = nops - 1;
        if (m->ops[fb.ab_gn].kind != OP_GNFIN || m->ops[fb.ab_qkv].kind != OP_CONV || m->ops[nops - 2].kind != OP_ATTN ||
            m->ops[fb.ab_outc].kind != OP_CONV)
          return fail("attention block plan out of order");
        fb.win_name = ap + ".mhsa.in_proj_weight"; fb.wout_name = ap + ".mhsa.out_proj.weight";
        if (upload(m, P(m, fb.win_name).host, &fb.d_win)) return 1;
        if (upload(m, P(m, fb.wout_name).host, &fb.d_wout)) return 1;
        if (m->precision == CM_PRECISION_F32 && !cm::diag_env("CM_NO_H2") && cm::attn_sample_ok(fb.S, fb.E, ATTN_HEADS, GN_GROUPS)) {
          std::vector<float> fi, fo;
          attn_pack_h2(P(m, fb.win_name).host.data(), P(m, fb.wout_name).host.data(), fb.E, &fi, &fo, &fb.ab_in_oscale, &fb.ab_out_oscale);
          if (upload(m, fi, &fb.d_win_h2) || upload(m, fo, &fb.d_wout_h2)) return 1;
        }
        for (int i = nops - 4; i < nops; ++i) m->ops[i].in_attn_block = true;
        const size_t need = (size_t)ATTN_HEADS * m->cfg.max_batch * fb.S * fb.E;
        m->ks_scratch_floats = std::max(m->ks_scratch_floats, need);
        m->ops.push_back(fb);
      }
    }
    return 0;
  };

  // first conv (unet.py:32,142)
  Act *h = new_act(m, "first", c.base_channels, Zl[0], Yl[0], Xl[0], true, &rc);
  if (rc) return 1;
  {
    ConvSpec cf; cf.s0 = m->x8_act; cf.wname = "first.weight"; cf.bname = "first.bias"; cf.out = h; cf.Co = c.base_channels; cf.ci_valid = c.in_channels; cf.stats = true;
    if (add_conv(m, cf)) return 1;
    add_stats(m, h);
  }
  std::vector<Act *> outs{h};
  for (auto &b : m->enc) {
    if (b.kind == 0) {
      Act *r = nullptr;
      if (res_block(b, h, nullptr, &r)) return 1;
      h = r;
    } else {
      Act *d = new_act(m, b.prefix, b.cout, Zl[b.level + 1], Yl[b.level + 1], Xl[b.level + 1], true, &rc);
      if (rc) return 1;
      ConvSpec cd; cd.s0 = h; cd.stride = 2; cd.wname = b.prefix + ".downsample.weight"; cd.bname = b.prefix + ".downsample.bias"; cd.out = d; cd.Co = b.cout; cd.stats = true;
      if (add_conv(m, cd)) return 1;
      add_stats(m, d);
      h = d;
    }
    outs.push_back(h);
  }
  for (auto &b : m->bott) {
    Act *r = nullptr;
    if (res_block(b, h, nullptr, &r)) return 1;
    h = r;
  }
  for (auto &b : m->dec) {
    if (b.kind == 0) {
      Act *skip = outs.back();
      outs.pop_back();
      Act *r = nullptr;
      if (res_block(b, h, skip, &r)) return 1;  // torch.cat([h, out], dim=1): h first (unet.py:160)
      h = r;
    } else {
      const int l = b.level - 1;
      Act *u = new_act(m, b.prefix, b.cout, Zl[l], Yl[l], Xl[l], true, &rc);
      if (rc) return 1;
      ConvSpec cu; cu.s0 = h; cu.ups = 1; cu.wname = b.prefix + ".upsample.1.weight"; cu.bname = b.prefix + ".upsample.1.bias"; cu.out = u; cu.Co = b.cout; cu.stats = true;
      if (add_conv(m, cu)) return 1;
      add_stats(m, u);
      h = u;
    }
  }
  // final: GN -> SiLU -> conv (unet.py:118-122,164)
  {
    float *gnf = nullptr;
    if (add_gnfin(m, h, nullptr, "final.0.weight", "final.0.bias", &gnf)) return 1;
    auto eo = std::make_unique<Act>();
    eo->name = "final"; eo->C = 8; eo->Z = L; eo->Y = c.rows; eo->X = c.cols;
    if (dev_alloc(m, (void **)&eo->d, (size_t)c.max_batch * eo->V() * 8 * sizeof(float))) return 1;
    CM_DEV(m, hipMemset(eo->d, 0, (size_t)c.max_batch * eo->V() * 8 * sizeof(float)));
    m->eps_cl = eo->d;
    Act *eop = eo.get();
    m->act_by_name["final"] = eop;
    m->acts.push_back(std::move(eo));
    ConvSpec cf; cf.s0 = h; cf.gn = gnf; cf.silu = 1; cf.wname = "final.2.weight"; cf.bname = "final.2.bias"; cf.out = eop; cf.Co = c.out_channels;
    if (add_conv(m, cf)) return 1;
  }
  if (m->ks_scratch_floats && dev_alloc(m, (void **)&m->ks_scratch, 4 * m->ks_scratch_floats * sizeof(float))) return 1;
  return 0;
}

// Finish the plan of one conv (cm_model_finalize, after build_ops): the tile geometry of the kernel family add_conv prepared, with
// the fall-backs a grid may force.  Feasibility is known only with the geometry: a grid the Winograd tiles do not fit, or a first
// conv with more columns than the full-X tile holds, goes to the direct kernel (its fragments `wfrag` are packed for every conv;
// NB was fixed before packing), which gets its tile from pick_tile and its coordinate tables on the device.  Nothing here depends
// on a launch: the tile is chosen for TUNE_BATCH, the Winograd and first-conv pickers see only the grid.
int resolve_conv(cm_model *m, Op &op) {
  if (op.wino) {
    cm::ConvArgs a = op.ca;
    a.bs = 1;
    op.wino = cm::conv_wino_pick(a.Zo, a.Yo, a.Xo, &a.bz, &a.by, &a.bx);
    if (op.wino) {
      a.ntz = a.Zo / a.bz; a.nty = (a.Yo + a.by - 1) / a.by; a.ntx = (a.Xo + a.bx - 1) / a.bx;
      op.wino = cm::conv_wino_ok(a);
    }
    if (op.wino) {
      op.ca = a;
      op.MB = 4;                     // statistics slots per tile: the four (a, b) output sub-blocks
      return 0;
    }
  }
  if (op.first_k) {
    const cm::ConvArgs keep = op.ca;
    pick_tile_first(op);
    if (cm::conv_first_ok(op.ca, op.first_cin)) return 0;
    op.ca = keep;
    op.first_k = false;
  }
  pick_tile(op, TUNE_BATCH);
  std::vector<int> hv((size_t)cm::conv_halo_voxels(op.ca)), mt((size_t)32 * op.MB);
  if (hv.size() > 16384) return fail("halo box too large");
  cm::conv_build_tables(op.ca, op.MB, hv.data(), mt.data());
  if (dev_alloc(m, (void **)&op.d_hvtab, 16384 * sizeof(int))) return 1;
  if (dev_alloc(m, (void **)&op.d_mtab, 256 * sizeof(int))) return 1;
  CM_DEV(m, hipMemcpyAsync(op.d_hvtab, hv.data(), hv.size() * sizeof(int), hipMemcpyHostToDevice, m->stream));
  CM_DEV(m, hipMemcpyAsync(op.d_mtab, mt.data(), mt.size() * sizeof(int), hipMemcpyHostToDevice, m->stream));
  CM_DEV(m, hipStreamSynchronize(m->stream));
  op.ca.hvtab = op.d_hvtab;
  op.ca.mtab = op.d_mtab;
  return 0;
}

// ------------------------------------------------------------------------------
// which kernel a conv runs on, and on which operands
// ------------------------------------------------------------------------------
// add_conv decides what CAN run (the fragment sets it packs), resolve_conv fixes the geometry, conv_route decides what DOES run in
// a given context; the launchers then pick their own template instantiation.  Everything that needs to know the kernel or the
// operand form of a conv -- the FLOP accounting, the f16-tensor plan, the debug hooks -- asks here, and so does plan_forward (below),
// which decides the rest: which ops run, every tensor's statistics slots, who finalises each GroupNorm.  The launch code only executes.

// Bit mask of the op's tensors that are stored as _Float16 (ConvArgs::h16; plan_h16): half the bytes per element.  The training
// forward never sees them (training refuses f16 handles); with the skip conv fused in, its sources take the residual's place.
int h16_mask(const Op &op, bool train_fwd) {
  auto is16 = [&](const Act *t) { return t && t->h16 && !train_fwd; };
  const int io = (is16(op.in0) ? 1 : 0) | (is16(op.in1) ? 2 : 0) | (is16(op.out_act) ? 4 : 0);
  if (op.d_s2w && !train_fwd) return io | (is16(op.skip0) ? 16 : 0) | (is16(op.skip1) ? 32 : 0);
  return io | (is16(op.resid_act) ? 8 : 0);
}

// Pure function of the resolved op and the context: no device pointer is dereferenced (fragment pointers count as present /
// absent), no stream, no model.  (plan_conv withdraws the upsample conv's h2 form where no earlier op writes its source's slot statistics.)
ConvRoute conv_route(const Op &op, int precision, bool train_fwd, bool h2_stale, bool autocast = false) {
  static const bool no_train_qr = cm::diag_env("CM_NO_TRAIN_QR") != nullptr, no_train_b6 = cm::diag_env("CM_NO_TRAIN_B6") != nullptr;
  const bool infer = !train_fwd;
  // the six-term fragments serve the training forward as well (exact splits, fp32 accumulate; they follow every optimizer step);
  // relaxed fp32 plan: only their three leading cross terms, in the inference forward
  const bool six_ok = infer || !no_train_b6;
  const ConvForm six = (precision == CM_PRECISION_F32R && infer) ? FORM_B3 : FORM_B6;
  // default plan, layers with bounded input, inference-only fragments (Op::d_wfin_h2); raw debug operands are unbounded unless the caller says otherwise
  const bool h2 = precision == CM_PRECISION_F32 && infer && !h2_stale && !op.h2_off && (!op.dbg_raw || op.dbg_h2);
  auto form = [&](const float *w16, const float *w6, const float *wh2) {   // f16 fragments exist under the reduced-precision plan only
    return (w16 && infer) ? FORM_F16 : !w6 ? FORM_FP32 : (h2 && wh2) ? FORM_H2 : six;
  };
  const cm::ConvArgs &g = op.ca;
  if (op.skip_if_fused && infer) return {CONV_NONE, FORM_FP32};      // absorbed by the block's conv_2 (inference plan)
  // (training forward: the same whole-sample kernel in its six-term form -- it finalises the GroupNorm of its input from the
  //  producers' partials like the inference plan does; the gn_finalize op still runs there for the backward's mean / rstd rows)
  if (op.qr && (infer || (op.d_wqr_b6 && op.train_qr && !no_train_qr))) {
    cm::QrArgs q{};                  // the launcher's own predicate for its split forms (8 groups, channel bound, LDS fit)
    q.C0 = g.C0; q.C1 = g.C1; q.Co = g.Co; q.Y = g.Yo; q.X = g.Xo; q.groups = GN_GROUPS; q.raw = 1; q.wq6 = op.d_wqr_b6;
    return {CONV_QR, form(nullptr, cm::conv_qr2_b6_ok(q) ? op.d_wqr_b6 : nullptr, op.d_wqr_h2)};
  }
  if (op.ks > 1) return {CONV_KSPLIT, FORM_FP32};
  if (op.ups && (op.d_wups16 || !(op.d_wfrag16 && infer)))
    return {CONV_UPS, form(op.d_wups16, six_ok ? op.d_wups_b6 : nullptr, op.d_wups_h2)};
  if (op.wino && op.f16d && infer) return {CONV_F16D, FORM_F16};
  // autocast training forward: the layers that train on the Winograd route take its f16-operand form (fp32 activations, fp32 accumulation)
  if (op.wino && train_fwd && autocast && op.d_wwino16t) return {CONV_WINO, FORM_F16};
  if (op.wino)
    return {CONV_WINO, form(op.d_wwino16, (op.d_wwino_b6 && six_ok && cm::conv_wino_b6_ok(g.bz, g.by, g.bx, g.Co, g.Zo)) ? op.d_wwino_b6 : nullptr, op.d_wwino_h2)};
  if (op.first_k) return {CONV_FIRST, FORM_FP32};
  // The remaining launchers' predicates also read what run_conv fills in per launch, as null / non-null only; each is a fact of the
  // op and the context: statistics <=> stat_act, Dropout3d multipliers <=> training forward of a conv_2, fused skip conv <=> inference.
  static float set;
  cm::ConvArgs a = g;
  a.stat_part = op.stat_act ? &set : nullptr;
  a.pm = (train_fwd && op.pm_off >= 0) ? &set : nullptr;
  a.s2w = infer ? op.d_s2w : nullptr;
  a.h16 = h16_mask(op, train_fwd);
  if (op.small_n) {
    a.by = op.fin_by; a.bx = op.fin_bx;
    if (op.fin && cm::conv_fin_ok(a)) return {CONV_FIN, form(op.d_wfin16, op.d_wfin, op.d_wfin_h2)};
    return {CONV_SMALLN, FORM_FP32};
  }
  if (op.d_w1x1_16 && infer && cm::conv1x1_f16_ok(a, op.NB)) return {CONV_1X1_F16, FORM_F16};
  return {CONV_GENERIC, form(cm::conv_par_f16_variant(op.MB, op.NB, g.bz, g.by, g.bx) ? op.d_wfrag16 : nullptr, nullptr, nullptr)};
}

// The training backward of a conv (cm_train_host.inc) asks the same way: wgrad_route names the kernel of the weight gradient,
// dgrad_route that of the data gradient.  Same contract as conv_route -- the resolved op, the geometry bwd_geom derives from it, a
// context (fragment sets as present / absent) and the diagnostic switches as a value (BwdKnobs: the one reader of the backward's
// CM_DIAG variables, so that the self-test flips a switch without an environment).
struct BwdKnobs {
  bool no_wino = false, no_wino_b6 = false, no_train_b6 = false, no_train_qr = false, no_wino_wgrad = false, no_wgrad_zsplit = false,
       no_wgrad_pack = false, no_wgrad_par = false, no_wgrad_1x1 = false, no_wgrad_zs_kernel = false, wgrad_one_stream = false;
  // workgroups per weight-gradient launch.  Winograd: one workgroup per CU (80 KB image, 192 accumulators; with the weight gradients on
  // their own stream 128 / 192 / 256 / 512 -> 14.63 / 13.59 / 13.69 / 13.88 ms per step); generic: two per CU fit (62 KB LDS each; 768:
  // 26.0 ms, 512: 23.2 ms per step); two-plane: one per CU, fewest partial copies (128 / 256 / 512 / 1024: 16.84 / 16.30 / 16.46 / 16.75 ms)
  int wino_wgs = 192, wgs = 256, zs_wgs = 128, x1_wgs = 768, par_wgs = 1024;
};
BwdKnobs read_bwd_knobs() {
  BwdKnobs k;
  auto on = [](const char *name) { return cm::diag_env(name) != nullptr; };
  auto num = [](const char *name, int dflt) { const char *v = cm::diag_env(name); return v ? atoi(v) : dflt; };
  k.no_wino = on("CM_NO_WINO"); k.no_wino_b6 = on("CM_NO_WINO_B6"); k.no_train_b6 = on("CM_NO_TRAIN_B6"); k.no_train_qr = on("CM_NO_TRAIN_QR");
  k.no_wino_wgrad = on("CM_NO_WINO_WGRAD"); k.no_wgrad_zsplit = on("CM_NO_WGRAD_ZSPLIT"); k.no_wgrad_pack = on("CM_NO_WGRAD_PACK");
  k.no_wgrad_par = on("CM_NO_WGRAD_PAR"); k.no_wgrad_1x1 = on("CM_NO_WGRAD_1X1"); k.no_wgrad_zs_kernel = on("CM_NO_WGRAD_ZS_KERNEL");
  k.wgrad_one_stream = on("CM_WGRAD_ONE_STREAM");
  k.wino_wgs = num("CM_WGRAD_WINO_WGS", k.wino_wgs); k.wgs = num("CM_WGRAD_WGS", k.wgs); k.zs_wgs = num("CM_WGRAD_ZS_WGS", k.zs_wgs);
  k.x1_wgs = num("CM_WGRAD_1X1_WGS", k.x1_wgs); k.par_wgs = num("CM_WGRAD_PAR_WGS", k.par_wgs);
  return k;
}

// f16_frags: the f16 siblings of the Winograd fragments exist (cm_train_set_autocast has run with mode 1)
struct BwdCtx { int precision = CM_PRECISION_F32; bool autocast = false, f16_frags = false; int max_batch = 1, in_channels = 8, tx = 0;
                const Act *x8 = nullptr, *seed = nullptr; };   // the UNet's input (no data gradient) and the tensor the loss gradient lands in

// Geometry of a conv's backward, from the resolved op alone (tiles through pick_tile / conv_wino_pick: no device).
struct BwdGeom {
  bool first = false;          // the first conv: its input is data
  int Co = 0, Ci = 0;          // of the reference weight (Ci < C0 + C1 on the first conv only)
  // data gradient dA[.., Ci_pad] = conv(dY, W'), W'[ci][co][t'] = W[co][ci][flip t']: a stride-1 conv on the op's INPUT grid
  // (stride-2: of the zero-stuffed dY; upsample: on the upsampled grid, pooled afterwards); C0 = Cy, the channel stride of dY
  cm::ConvArgs da{};
  int dMB = 1, dNB = 1;
  bool dwino = false;          // ... a Winograd tile fits it (da then carries the tile)
  // weight gradient of the generic kernel: the op's own geometry, one sample per tile, 32-channel rows (the parity-mode upsample
  // conv keeps its 2x2x2 parity form: 8 taps on the low-resolution input); zsplit: two-plane grids in z-split row order -- plane z
  // in row block z -- so that the kernel can skip the z tap on the padding plane, as the forward's z-split form does (cm_conv.hip)
  cm::ConvArgs wa{};
  int wMB = 1;
  bool zsplit = false;
};

void tune_tile(cm::ConvArgs &ca, int &MB, int NB, bool wgrad) {
  Op tmp;
  tmp.kind = OP_CONV; tmp.ca = ca; tmp.NB = NB;
  static Act dummy;
  tmp.stat_act = wgrad ? &dummy : nullptr;  // the weight-gradient kernel wants one sample per tile
  if (wgrad) tmp.ca.CK = 32;                 // ... and stages 32-channel rows whatever the forward chunking
  pick_tile(tmp, TUNE_BATCH);
  const int ck = ca.CK;
  ca = tmp.ca; ca.CK = ck; MB = tmp.MB;
}

// train_setup keeps the Winograd fragments of a data gradient by these two, the route below launches by them
bool dgrad_wino_ok(const BwdGeom &g, const BwdKnobs &k) { return g.dwino && !k.no_wino; }
bool dgrad_wino_b6(const BwdGeom &g, const BwdCtx &ctx, const BwdKnobs &k) {
  return dgrad_wino_ok(g, k) && ctx.precision != CM_PRECISION_F16 && !k.no_wino_b6 && !k.no_train_b6 &&
         cm::conv_wino_b6_ok(g.da.bz, g.da.by, g.da.bx, g.Ci, g.da.Zo);
}

BwdGeom bwd_geom(const Op &op, const BwdCtx &ctx, const BwdKnobs &k) {
  BwdGeom g;
  const int nt = op.ref_taps, Cy = op.out_act->C, Ci_pad = op.ca.C0 + op.ca.C1;
  g.first = op.in0 == ctx.x8; g.Co = op.ca.Co; g.Ci = g.first ? ctx.in_channels : Ci_pad;
  cm::ConvArgs &a = g.da;
  a.C0 = Cy; a.C1 = 0; a.Co = g.Ci;
  a.ntaps = nt; a.td = nt == 27 ? 3 : 1; a.stride = 1; a.ups = 0; a.par = 0; a.ks = 1;
  const int up = op.ca.par ? 2 : 1;
  a.Zs = a.Zo = op.ca.Zs * up; a.Ys = a.Yo = op.ca.Ys * up; a.Xs = a.Xo = op.ca.Xs * up;
  a.out_cs = Ci_pad; a.CK = pick_ck(Cy, 0);
  a.nch0 = a.CK ? Cy / a.CK : 0; a.nch1 = 0;
  g.dNB = g.Ci > 32 ? 2 : 1;
  int wz = 0, wy = 0, wx = 0;
  g.dwino = !g.first && nt == 27 && Cy % 16 == 0 && g.Ci % 32 == 0 && g.Ci == Ci_pad && (long)a.Zo * a.Yo * a.Xo > 64 &&
            cm::conv_wino_pick(a.Zo, a.Yo, a.Xo, &wz, &wy, &wx);
  if (dgrad_wino_ok(g, k)) {
    a.bs = 1; a.bz = wz; a.by = wy; a.bx = wx;
    a.ntz = a.Zo / wz; a.nty = (a.Yo + wy - 1) / wy; a.ntx = (a.Xo + wx - 1) / wx;
  } else if (!g.first) tune_tile(a, g.dMB, g.dNB, false);
  cm::ConvArgs &wa = g.wa;
  wa = op.ca; wa.ks = 1;
  tune_tile(wa, g.wMB, 1, true);
  g.zsplit = wa.ntaps == 27 && wa.stride == 1 && !wa.par && !wa.ups && wa.Zo == 2 && wa.Zs == 2 && wa.bz == 2 && wa.by * wa.bx <= 32 && !k.no_wgrad_zsplit;
  return g;
}

enum WgradKernel { WG_WINO, WG_PACK, WG_PAR, WG_1X1, WG_ZS, WG_GENERIC };
enum DgradKernel { DG_NONE, DG_QR, DG_WINO, DG_GENERIC };
struct WgradRoute { WgradKernel kernel; ConvForm form; };   // FORM_F16 on the Winograd kernel under autocast, FORM_FP32 otherwise
struct DgradRoute { DgradKernel kernel; ConvForm form; };   // Winograd: FP32 / B6 / F16; conv_qr2: B6 (its six-term form, raw source)

WgradRoute wgrad_route(const Op &op, const BwdGeom &g, const BwdCtx &ctx, const BwdKnobs &k) {
  const cm::ConvArgs &a = op.ca;
  const bool plain27 = op.ref_taps == 27 && a.stride == 1 && !a.par && !a.ups;
  // the forward op is a Winograd layer: weight gradient in the Winograd domain, on f16 operands under autocast
  if (op.wino && g.Ci % 32 == 0 && g.Co % 32 == 0 && !k.no_wino_wgrad) return {WG_WINO, (ctx.autocast && ctx.f16_frags) ? FORM_F16 : FORM_FP32};
  // few channels on one side (first / last conv of the UNet): taps packed with the narrow side into the MFMA columns
  if (plain27 && op.pm_off < 0 && !k.no_wgrad_pack &&
      ((a.Co == 32 && !op.in1 && op.in0->C == 8 && !a.gn) || (a.Co <= 4 && a.C0 + a.C1 == 32 && !op.in1))) return {WG_PACK, FORM_FP32};
  // upsample convs: parity-form kernel with all 8 tap blocks per wave
  if (a.par && !a.gn && op.pm_off < 0 && !k.no_wgrad_par) return {WG_PAR, FORM_FP32};
  // 1x1x1 convs (skip convs, attention projections): flat-row kernel, NKB input blocks per workgroup
  if (op.ref_taps == 1 && a.stride == 1 && !a.par && !a.ups && !k.no_wgrad_1x1) return {WG_1X1, FORM_FP32};
  // two-plane grids: the dedicated kernel (two input blocks per workgroup, arithmetic coordinates, one load batch per tile)
  if (g.zsplit && !k.no_wgrad_zs_kernel && cm::wgrad_zs_ok(g.wa)) return {WG_ZS, FORM_FP32};
  return {WG_GENERIC, FORM_FP32};
}

// conv_qr2's six-term form holds both launches of a quarter-resolution conv's training step: the forward on the op's own sources
// (conv_route takes the kernel there exactly where the data gradient does: Op::train_qr) and the data gradient on dY.  Asked here, so
// that a width or a plane the form cannot hold trains on the generic kernels instead of failing inside its first step.
bool train_qr_forms_ok(const Op &op, const BwdGeom &g) {
  cm::QrArgs f{}, d{};
  f.C0 = op.ca.C0; f.C1 = op.ca.C1; f.Co = op.ca.Co; f.Y = op.ca.Yo; f.X = op.ca.Xo; f.groups = GN_GROUPS; f.raw = 1; f.wq6 = op.d_wqr_b6;
  d.C0 = g.da.C0; d.Co = g.da.Co; d.Y = g.da.Yo; d.X = g.da.Xo; d.groups = 8; d.raw = 1; d.wq6 = op.d_wqr_b6; d.out_cs = g.da.out_cs;
  return cm::conv_qr2_b6_ok(f) && cm::conv_qr2_b6_ok(d);
}

DgradRoute dgrad_route(const Op &op, const BwdGeom &g, const BwdCtx &ctx, const BwdKnobs &k) {
  if (g.first) return {DG_NONE, FORM_FP32};
  const cm::ConvArgs &a = g.da;
  const int Cy = a.C0, Ci_pad = a.out_cs;
  // quarter resolution (two planes): forward and data gradient of the training step on conv_qr2's six-term form
  if (op.qr && op.d_wqr_b6 && op.ref_taps == 27 && Cy == g.Co && g.Co % 64 == 0 && g.Ci % 32 == 0 && g.Ci == Ci_pad && a.Zo == 2 &&
      a.Yo * a.Xo <= 64 && 8 * (a.Yo + 2) * (a.Xo + 2) <= 64 * 9 && ctx.precision != CM_PRECISION_F16 && !k.no_train_qr && train_qr_forms_ok(op, g))
    return {DG_QR, FORM_B6};
  // the data gradient of a 3x3x3 conv is a stride-1 3x3x3 conv of dY with the flipped / transposed weights: same Winograd kernel.
  // fp32 plan: the six-term bf16 form wherever the forward's tile takes it (exact three-way splits, fp32 accumulate: fp32-level
  // products at 2.7x the matrix rate); autocast: f16 operands
  if (dgrad_wino_ok(g, k)) {
    if (ctx.autocast && ctx.f16_frags) return {DG_WINO, FORM_F16};
    return {DG_WINO, dgrad_wino_b6(g, ctx, k) ? FORM_B6 : FORM_FP32};
  }
  return {DG_GENERIC, FORM_FP32};
}

// Which routes read / write tensors stored as _Float16, by the launch's tensor mask (h16_mask): the direct f16 conv (source, residual,
// fused skip source, output), the f16 stage-once upsample conv (source, output), the first conv (output), the last conv (sources).
// plan_h16 flags a tensor only when every kernel around it passes; plan_forward refuses a launch that does not.
bool route_takes_h16(ConvRoute r, int mask) {
  switch (r.kernel) {
    case CONV_F16D: return true;
    case CONV_UPS: return r.form == FORM_F16 && !(mask & ~5);
    case CONV_FIRST: return !(mask & ~4);
    case CONV_FIN: case CONV_SMALLN: return !(mask & ~3);
    default: return false;
  }
}

// The two ends of the UNet inside cm_sample_loop.  The z axis is the frame axis: P past frames, then F noisy ones; a loop step reads
// only the output's future planes, and rewrites only the input's.  Decided here, once per loop call, from the routes of the two convs:
//   * tz_first: the first conv (CONV_FIRST: no GroupNorm, time row or residual in front of it) launches z tiles [tz_first, ntz) in
//     every step but the call's first -- the tiles below compute from past frames alone, and their outputs and statistics slots stay
//     where step 0 left them (every activation has its own allocation).  Only when the resolved tile height divides P - 1.
//   * zo_first / zo_end: the last conv (CONV_FIN) computes output planes [P, P + F) only.
//   * fuse: it also applies the reverse-process update to them (variant 1 or 2 of launch_conv_fin); the loop then launches no
//     sampler_step_kernel and eps_cl is not written.  Mass-preservation guidance still runs afterwards, on the new x.
// A DiT handle, a last conv on conv_smalln (other channel counts, odd grids) or a first conv on the generic kernel keep the whole
// launch and the separate sampler kernel.  Nothing here outlives the loop call.
struct LoopEnds {
  int tz_first = 0;
  int zo_first = 0, zo_end = 0;
  int fuse = 0;
  const cm::StepArgs *step = nullptr;   // per step and lane: the update's arguments (fuse != 0)
};
LoopEnds loop_ends_plan(const std::vector<Op> &ops, const float *x8, const float *eps_cl, int mask, int precision, bool h2_stale, int P, int F,
                        int Cin, int Cout) {
  LoopEnds le;
  for (const Op &op : ops) {
    if (op.kind != OP_CONV) continue;
    const ConvRoute r = conv_route(op, precision, false, h2_stale);
    if (r.kernel == CONV_FIRST && op.ca.src0 == x8 && (mask & 4)) le.tz_first = cm::conv_first_const_ztiles(op.ca.bz, op.ca.ntz, P);
    if (r.kernel == CONV_FIN && op.ca.out == eps_cl && op.ca.Zo == P + F && (mask & 3)) {
      le.zo_first = P; le.zo_end = P + F;
      // (the update addresses x by the conv's channels: one tensor geometry for both; LDS rows for at most 8 frames)
      if ((mask & 2) && Cin == Cout && op.ca.Co == Cout && op.ca.out_cs == 8 && F <= 8) le.fuse = (mask & 8) ? 2 : 1;
    }
  }
  return le;
}

// f16 ACTIVATIONS (round 4; reduced-precision plan = BASELINE configs[4]; the reference's autocast stores every conv output as
// fp16, ddpm.py:116-120): a tensor is stored as _Float16 when the kernel that produces it can write f16 and every kernel that reads
// it can read f16 (route_takes_h16).  That covers the full- and half-resolution tensors of a grid with >= 4
// planes at half resolution except the inputs of the two stride-2 convs; quarter-resolution tensors (2 % of the bytes) stay fp32.
// GroupNorm statistics come from the fp32 accumulators of the producer; a kernel that cannot honour a flagged tensor fails loudly
// (run_conv) instead of misreading it.  CM_NO_H16 under CM_DIAG=1 keeps fp32 storage (A/B runs).
int plan_h16(cm_model *m) {
  if (m->precision != CM_PRECISION_F16 || cm::diag_env("CM_NO_H16")) return 0;
  auto takes = [&](const Op &o, int role) { return route_takes_h16(conv_route(o, m->precision, false, false), role); };
  for (auto &ap : m->acts) {
    Act *a = ap.get();
    bool ok = false;
    for (const Op &o : m->ops)
      if (o.kind == OP_CONV && o.out_act == a && !o.skip_if_fused) ok = takes(o, 4);
    for (const Op &o : m->ops) {
      if (!ok) break;
      if (o.kind == OP_ATTNBLK && o.ab_x == a) ok = false;
      if (o.kind == OP_ATTN && (o.qkv == a->d || o.aout == a->d)) ok = false;
      if (o.kind != OP_CONV || o.skip_if_fused) continue;       // (the stand-alone skip conv: absorbed by the block's conv_2 at inference)
      const int role = (o.in0 == a ? 1 : 0) | (o.in1 == a ? 2 : 0) | (o.resid_act == a ? 8 : 0) | (o.skip0 == a ? 16 : 0) | (o.skip1 == a ? 32 : 0);
      if (role) ok = takes(o, role);
    }
    a->h16 = ok;
  }
  return 0;
}

// The conv part of a plan entry: the op's route in `ctx` and the slot count of the statistics it writes, that of the kernel family that
// runs.  `src_slots`: slots an earlier op writes for the source tensor (the upsample conv's h2 form reads them), 0 = none.  Returns an error text or "".
std::string plan_conv(const Op &op, const FwdCtx &ctx, int src_slots, OpPlan *p) {
  ConvRoute r = conv_route(op, ctx.precision, ctx.train_fwd, ctx.h2_stale, ctx.autocast);
  if (r.kernel == CONV_UPS && r.form == FORM_H2 && src_slots <= 0) {
    Op plain = op; plain.d_wups_h2 = nullptr;
    r = conv_route(plain, ctx.precision, ctx.train_fwd, ctx.h2_stale);
  }
  p->route = r; p->launch = r.kernel != CONV_NONE; p->ns_out = 0; p->ns0 = src_slots;
  // only some kernels read / write f16 tensors (plan_h16); anything else would misread them silently
  const int h16 = h16_mask(op, ctx.train_fwd);
  if (p->launch && h16 && r.kernel != CONV_QR && !route_takes_h16(r, h16))
    return "conv " + op.label + ": f16 tensors (mask " + std::to_string(h16) + ") reach a kernel without f16 tensor support";
  if (!p->launch || !op.stat_act) return "";
  cm::ConvArgs a = op.ca;
  int ns = a.ntz * a.nty * a.ntx * op.MB * (a.par ? 8 : 1);                      // of the resolved tile, unless:
  if (r.kernel == CONV_QR) ns = a.Yo * a.Xo > 32 ? 4 : 2;
  if (r.kernel == CONV_KSPLIT) ns = (a.Zo * a.Yo * a.Xo + 31) / 32;             // of the combine pass: one per 32 voxels
  if (r.kernel == CONV_UPS) { a.bz = op.ups_tz; a.by = op.ups_ty; a.bx = op.ups_tx; ns = cm::conv_ups_slots(a, op.ups_mbw); }
  if (r.kernel == CONV_F16D) { a.bz = op.f16d_bz; a.by = op.f16d_by; a.bx = op.f16d_bx; ns = cm::conv_f16d_slots(a, op.f16d_mbw); }
  if (ns < 1 || ns > MAX_SLOTS) return "conv " + op.label + ": " + std::to_string(ns) + " statistics slots, outside [1, " + std::to_string(MAX_SLOTS) + "]";
  p->ns_out = ns;
  return "";
}

// Does conv `c` on route `r` merge the slot partials behind its GroupNorm itself at batch B?  Only conv_wino_p_kernel does (the launcher's own test)
bool wino_merges(const Op &c, ConvRoute r, int B) {
  cm::ConvArgs a = c.ca;
  a.B = B; a.f16 = r.form == FORM_F16 ? a.f16 : (int)r.form;
  return r.kernel == CONV_WINO && r.form != FORM_FP32 && a.gn && cm::conv_wino_p_taken(a, r.form == FORM_F16, true);
}

// Does an OP_ATTNBLK of this context qualify for the whole-sample launch (attn_sample_kernel: both projections in the h2 form)?  The
// default plan's inference forward with current fragments, like every h2 conv; plan_forward adds: no finalisation carried.
bool attn_sample_planned(const Op &op, const FwdCtx &ctx) {
  static const bool off = cm::diag_env("CM_NO_ATTN_SAMPLE") != nullptr;
  return !off && !ctx.train_fwd && ctx.precision == CM_PRECISION_F32 && !ctx.h2_stale && op.d_win_h2 && op.d_wout_h2 &&
         op.ab_in_oscale > 0.f && op.ab_out_oscale > 0.f && cm::attn_sample_ok(op.S, op.E, ATTN_HEADS, GN_GROUPS);
}

// Everything the launches of one forward depend on, in one walk over the op list: which ops run, each conv's route, every tensor's
// statistics slot count, one disposition (FinBy) per GroupNorm finalisation.  Pure: no device memory, no stream, no model state --
// only, through conv_wino_p_taken under the f16 plan, the current device's CU count (256 where there is no device: the self-test).
FwdPlan plan_forward(const std::vector<Op> &ops, const FwdCtx &ctx) {
  static const bool no_fuse = cm::diag_env("CM_NO_FUSE_GNFIN") != nullptr, no_slot_gn = cm::diag_env("CM_NO_SLOT_GN") != nullptr;
  FwdPlan P{ctx, std::vector<OpPlan>(ops.size()), ""};
  const bool infer = !ctx.train_fwd; const int n = (int)ops.size();
  std::map<const Act *, int> slots;      // per tensor: what the launched ops walked so far write
  auto slots_of = [&](const Act *t) { return slots.count(t) ? slots[t] : 0; };
  // the fused attention block runs in the inference plan, its four generic ops in the training forward
  auto in_ctx = [&](const Op &o) { return o.kind == OP_ATTNBLK ? infer : !(o.in_attn_block && infer); };
  for (int i = 0; i < n && P.err.empty(); ++i) {
    const Op &op = ops[i];
    OpPlan &p = P.ops[i];
    if (!in_ctx(op)) continue;
    p.launch = op.kind != OP_GNFIN;
    const Act *two_pass = nullptr; int pc = 0, pv = 0;   // output (channels, voxels) of a K-split conv / attention block: its second pass can carry a finalisation
    if (op.kind == OP_CONV) {
      P.err = plan_conv(op, ctx, (op.in0 && op.in0->part) ? slots_of(op.in0) : 0, &p);
      if (p.ns_out) slots[op.stat_act] = p.ns_out;
      if (p.route.kernel == CONV_KSPLIT) { two_pass = op.stat_act; pc = op.ca.Co; pv = op.ca.Zo * op.ca.Yo * op.ca.Xo; }
    } else if (op.kind == OP_STATS) {
      slots[op.act] = p.ns_out = op.act->nslice;
    } else if (op.kind == OP_ATTNBLK) {
      slots[op.ab_out] = p.ns_out = (op.S + 31) / 32; two_pass = op.ab_out; pc = op.E; pv = op.S;
    } else if (op.kind == OP_GNFIN && p.fin != FIN_COMBINE) {      // (FIN_COMBINE: decided at its producer, below)
      p.ns0 = slots_of(op.g0); p.ns1 = op.g1 ? slots_of(op.g1) : 0;
      if (p.ns0 < 1 || (op.g1 && p.ns1 < 1)) P.err = op.label + ": no earlier op of the forward writes its statistics";
      int cons = -1, ncons = 0;
      for (int j = i + 1; j < n; ++j) if (ops[j].kind == OP_CONV && ops[j].gn_op == i) { cons = j; ++ncons; }
      // few slots and a single consumer on the table-driven Winograd kernel: it merges them in its prologue
      // (<= 16 slots: measured -0.7 % on the ATC step, -1.6 % on the 24x72 f16 plan; HERMES-CR-120's half resolution has 24 slots
      //  per tensor and up to 192 channels -- there the merge in 256 workgroups cost more than the launch, +0.5 %)
      const bool merge = ncons == 1 && infer && !no_slot_gn && p.ns0 <= 16 && (!op.g1 || (p.ns1 <= 16 && op.g1->V() == op.g0->V())) &&
                         wino_merges(ops[cons], conv_route(ops[cons], ctx.precision, false, ctx.h2_stale), ctx.B);
      p.fin = (op.qr_consumer && infer) ? FIN_QR : merge ? FIN_WINO : FIN_ALONE; p.launch = p.fin == FIN_ALONE;   // (FIN_QR: cm_conv_qr.hip finalises its own input)
    }
    // the next op of this context, when it finalises the tensor just produced: in the second pass (cm::launch_combine_gn, with the
    // mean / rstd rows when training), if the launcher's own predicate takes the geometry
    int j = i + 1;
    while (j < n && !in_ctx(ops[j])) ++j;
    if (two_pass && !no_fuse && j < n && ops[j].kind == OP_GNFIN && ops[j].g0 == two_pass && !(ops[j].qr_consumer && infer)) {
      const Act *g1 = ops[j].g1;
      cm::CombineArgs cb{};
      cb.C = pc; cb.V = pv; cb.B = ctx.B; cb.nslots = p.ns_out; cb.stat_part = two_pass->part; cb.fin_C1 = g1 ? g1->C : 0; cb.fin_groups = GN_GROUPS;
      if (!(g1 && (g1->V() != pv || slots_of(g1) < 1)) && cm::combine_gn_ok(cb)) {
        p.carries = j; P.ops[j].fin = FIN_COMBINE; P.ops[j].ns0 = p.ns_out; P.ops[j].ns1 = g1 ? slots_of(g1) : 0;
      }
    }
    // the attention block as one whole-sample launch: nothing for a second pass to carry, so only where none is planned
    if (op.kind == OP_ATTNBLK) p.attn_sample = attn_sample_planned(op, ctx) && p.carries < 0;
  }
  return P;
}

// Time-embedding tables for all 1000 rows (embeddings.py:24-30 + layers.py:35,62).
int build_time_table(cm_model *m) {
  const cm_unet_config &c = m->cfg;
  const int te = c.base_channels, tx = c.base_channels * c.time_multiple;
  std::vector<float> Wd((size_t)m->nproj * tx), bd((size_t)m->nproj);
  int off = 0;
  auto visit = [&](const BlockDesc &b) {
    if (b.kind != 0) return;
    const Param &w = P(m, b.prefix + ".dense_1.weight");
    const Param &bb = P(m, b.prefix + ".dense_1.bias");
    std::copy(w.host.begin(), w.host.end(), Wd.begin() + (size_t)off * tx);
    std::copy(bb.host.begin(), bb.host.end(), bd.begin() + off);
    off += b.cout;
  };
  for (auto &b : m->enc) visit(b);
  for (auto &b : m->bott) visit(b);
  for (auto &b : m->dec) visit(b);
  float *dT, *dW1, *db1, *dW2, *db2, *dWd, *dbd;
  if (upload(m, P(m, "time_embeddings.time_blocks.0.weight").host, &dT)) return 1;
  if (upload(m, P(m, "time_embeddings.time_blocks.1.weight").host, &dW1)) return 1;
  if (upload(m, P(m, "time_embeddings.time_blocks.1.bias").host, &db1)) return 1;
  if (upload(m, P(m, "time_embeddings.time_blocks.3.weight").host, &dW2)) return 1;
  if (upload(m, P(m, "time_embeddings.time_blocks.3.bias").host, &db2)) return 1;
  if (upload(m, Wd, &dWd)) return 1;
  if (upload(m, bd, &dbd)) return 1;
  m->d_time[0] = dT; m->d_time[1] = dW1; m->d_time[2] = db1; m->d_time[3] = dW2; m->d_time[4] = db2;
  m->d_time[5] = dWd; m->d_time[6] = dbd;
  CM_HIP(cm::launch_time_mlp(dT, dW1, db1, dW2, db2, dWd, dbd, te, tx, m->nproj, TIME_ROWS, nullptr, m->temb_table, nullptr, m->stream));
  CM_HIP(hipStreamSynchronize(m->stream));
  return 0;
}

// ------------------------------------------------------------------------------
// forward: the launch code executes a plan (plan_forward) and writes nothing into the op list
// ------------------------------------------------------------------------------
// `ns` slots of tensor t's statistics for the samples from b0: (partials, rows behind each slot)
float *slot_part(const Act *t, int ns, int b0) { return t->part + (size_t)b0 * ns * t->C * 2; }
float *slot_cnt(const Act *t, int ns, int b0) { return t->cnt + (size_t)b0 * ns; }

// the stand-alone GroupNorm finalisation `g` (an OP_GNFIN, plan entry `gp`) for the `B` samples from `b0`
int run_gnfin(const Op &g, const OpPlan &gp, int B, hipStream_t st, int b0) {
  const Act *g0 = g.g0, *g1 = g.g1; const int Ct = g0->C + (g1 ? g1->C : 0);
  if (g1 && g1->V() != g0->V()) return fail("concat sources disagree on voxel count");
  CM_HIP(cm::launch_gn_finalize(slot_part(g0, gp.ns0, b0), slot_cnt(g0, gp.ns0, b0), gp.ns0, g0->C,
                                g1 ? slot_part(g1, gp.ns1, b0) : nullptr, g1 ? slot_cnt(g1, gp.ns1, b0) : nullptr,
                                g1 ? gp.ns1 : 0, g1 ? g1->C : 0, g0->V(), g.gamma, g.beta, GN_GROUPS, GN_EPS,
                                g.gn_out + (size_t)b0 * 2 * Ct, g.gn_mr ? g.gn_mr + (size_t)b0 * 2 * Ct : nullptr, B, st));
  return 0;
}

// Second pass of a K-split layer (or the head sum of the fused attention block) for the samples from b0: with the GroupNorm
// finalisation of the op that consumes its output when the plan says it carries one (`fin` = OpPlan::carries >= 0)
int run_combine(cm::CombineArgs &cb, const std::vector<Op> &ops, const FwdPlan &plan, int fin, int b0, hipStream_t st) {
  if (fin >= 0) {
    const Op &f = ops[fin];
    const Act *g1 = f.g1;
    const int Ct = cb.C + (g1 ? g1->C : 0), ns1 = plan.ops[fin].ns1;
    cb.fin_gamma = f.gamma; cb.fin_beta = f.beta;
    cb.fin_gn = f.gn_out + (size_t)b0 * 2 * Ct; cb.fin_mr = f.gn_mr ? f.gn_mr + (size_t)b0 * 2 * Ct : nullptr;
    if (g1) { cb.fin_p1 = slot_part(g1, ns1, b0); cb.fin_n1 = slot_cnt(g1, ns1, b0); cb.fin_ns1 = ns1; cb.fin_C1 = g1->C; }
    cb.fin_groups = GN_GROUPS; cb.fin_eps = GN_EPS;
  }
  CM_HIP(fin >= 0 ? cm::launch_combine_gn(cb, st) : cm::launch_ksplit_combine(cb, st));
  return 0;
}

// the whole-sample kernel of the lowest resolution: the GroupNorm statistics of its sources come raw (FIN_QR)
int run_conv_qr(const cm_model *m, const Op &op, const FwdPlan &plan, const OpPlan &p, hipStream_t st, int b0) {
  const Op &gop = m->ops[op.gn_op]; const OpPlan &gp = plan.ops[op.gn_op];
  const Act *g0 = gop.g0, *g1 = gop.g1;
  const cm::ConvArgs &ca = op.ca;
  const bool train = plan.ctx.train_fwd; const size_t V = (size_t)ca.Zo * ca.Yo * ca.Xo;
  cm::QrArgs q{};
  q.src0 = ca.src0 + (size_t)b0 * V * ca.C0; q.C0 = ca.C0;
  q.src1 = ca.src1 ? ca.src1 + (size_t)b0 * V * ca.C1 : nullptr; q.C1 = ca.C1;
  q.part0 = slot_part(g0, gp.ns0, b0); q.cnt0 = slot_cnt(g0, gp.ns0, b0); q.ns0 = gp.ns0;
  if (g1) { q.part1 = slot_part(g1, gp.ns1, b0); q.cnt1 = slot_cnt(g1, gp.ns1, b0); q.ns1 = gp.ns1; }
  if (g0->C != ca.C0 || (g1 ? g1->C : 0) != ca.C1) return fail("quarter-resolution conv %s: statistics and sources disagree", op.label.c_str());
  q.gamma = gop.gamma; q.beta = gop.beta; q.groups = GN_GROUPS; q.eps = GN_EPS; q.silu = ca.silu;
  if (op.dbg_raw) { q.gamma = q.beta = nullptr; q.raw = 1; q.silu = 0; }
  q.wq = op.d_wqr; q.bias = ca.bias;
  q.wq6 = op.d_wqr_b6;
  q.three = p.route.form == FORM_B3 ? 1 : 0;
  // default plan, inference-only handle: the f16 two-way-split form (bounded input: GroupNorm + SiLU inside the kernel)
  if (p.route.form == FORM_H2) { q.wq6 = op.d_wqr_h2; q.three = 2; q.h2_oscale = op.h2_oscale; }
  q.temb = ca.temb; q.temb_stride = ca.temb_stride; q.tidx = ca.tidx + b0;
  q.resid = ca.resid ? ca.resid + (size_t)b0 * V * ca.res_cs : nullptr; q.res_cs = ca.res_cs;
  if (train) {
    // training forward (six-term form only, see run_conv): Dropout3d multipliers on the activated input, the time-embedding rows
    // of this batch, the block's skip conv as its own op (its output arrives as the residual)
    if (op.pm_off >= 0) { q.pm = m->dropmask + (size_t)b0 * m->nproj + op.pm_off; q.pm_stride = m->nproj; }
    if (m->use_train_temb && op.temb_off >= 0) { q.temb = m->train_temb + op.temb_off; q.tidx = m->train_iota + b0; }
  } else if (op.d_wqr_skip) {
    q.s2w = op.d_wqr_skip;
    q.s2src0 = op.skip0->d + (size_t)b0 * V * op.skip0->C; q.s2C0 = op.skip0->C;
    q.s2src1 = op.skip1 ? op.skip1->d + (size_t)b0 * V * op.skip1->C : nullptr; q.s2C1 = op.skip1 ? op.skip1->C : 0;
    q.resid = nullptr;
    q.bias = op.d_bias_fused;
  }
  q.out = ca.out + (size_t)b0 * V * ca.out_cs; q.out_cs = ca.out_cs; q.Co = ca.Co; q.B = plan.ctx.B; q.Y = ca.Yo; q.X = ca.Xo;
  q.stat_C = op.stat_act->C; q.stat_part = slot_part(op.stat_act, p.ns_out, b0); q.stat_cnt = slot_cnt(op.stat_act, p.ns_out, b0);
  if (train && !cm::conv_qr2_b6_ok(q)) return fail("quarter-resolution conv %s: no six-term form for the training forward", op.label.c_str());
  CM_HIP(cm::launch_conv_qr(q, st));
  return 0;
}

// One convolution op of the list (plan entry `p`) for the plan's batch of samples starting at `b0` (see run_ops).
int run_conv(const cm_model *m, const Op &op, const FwdPlan &plan, const OpPlan &p, hipStream_t st, int b0, int slab, const LoopEnds *le = nullptr) {
  const ConvRoute route = p.route;
  const bool train = plan.ctx.train_fwd; const int B = plan.ctx.B;
  if (route.kernel == CONV_NONE) return 0;
  if (route.kernel == CONV_QR) return run_conv_qr(m, op, plan, p, st, b0);
  cm::ConvArgs ca = op.ca;
  ca.B = B;
  ca.nts = (B + ca.bs - 1) / ca.bs;
  const size_t Vs = (size_t)ca.Zs * ca.Ys * ca.Xs, Vo = (size_t)ca.Zo * ca.Yo * ca.Xo;
  // f16 tensors of the reduced-precision plan (plan_h16): half the bytes per element, so half the float offset; the mask tells the
  // kernel which of its tensors they are
  ca.h16 = h16_mask(op, train);
  auto adv = [&](auto *ptr, size_t elems, int bit) { return ptr + ((ca.h16 & bit) ? elems / 2 : elems); };
  ca.src0 = adv(ca.src0, (size_t)b0 * Vs * ca.C0, 1);
  if (ca.src1) ca.src1 = adv(ca.src1, (size_t)b0 * Vs * ca.C1, 2);
  if (ca.gn) ca.gn += (size_t)b0 * 2 * (ca.C0 + ca.C1);
  ca.tidx += b0;
  if (train && op.pm_off >= 0) { ca.pm = m->dropmask + (size_t)b0 * m->nproj + op.pm_off; ca.pm_stride = m->nproj; }
  if (m->use_train_temb && op.temb_off >= 0) { ca.temb = m->train_temb + op.temb_off; ca.tidx = m->train_iota + b0; }
  if (ca.resid) ca.resid = adv(ca.resid, (size_t)b0 * Vo * ca.res_cs, 8);
  if (op.d_s2w && !train) {
    if (!op.wino && 32 * op.MB > cm::conv_halo_voxels(ca)) return fail("fused skip conv: tile rows exceed the staged box");
    ca.s2w = op.d_s2w;
    ca.s2src0 = adv((const float *)op.skip0->d, (size_t)b0 * Vo * op.skip0->C, 16); ca.s2C0 = op.skip0->C;
    ca.s2src1 = op.skip1 ? adv((const float *)op.skip1->d, (size_t)b0 * Vo * op.skip1->C, 32) : nullptr; ca.s2C1 = op.skip1 ? op.skip1->C : 0;
    ca.resid = nullptr;
    ca.bias = op.d_bias_fused;
  }
  ca.out = adv(ca.out, (size_t)b0 * Vo * ca.out_cs, 4);
  if (op.stat_act) {   // statistics slots of the output tensor: the plan's count for the kernel that runs
    ca.stat_C = op.stat_act->C; ca.stat_ns = p.ns_out;
    ca.stat_part = slot_part(op.stat_act, p.ns_out, b0); ca.stat_cnt = slot_cnt(op.stat_act, p.ns_out, b0);
  }
  switch (route.kernel) {
    case CONV_NONE: case CONV_QR: break;   // (taken above)
    case CONV_KSPLIT: {
      cm::ConvArgs ka = ca;
      const int V = op.out_act->V();
      float *scratch = m->ks_scratch + (size_t)slab * m->ks_scratch_floats;
      ka.temb = nullptr; ka.resid = nullptr; ka.stat_part = nullptr; ka.bias = op.d_zero_bias;
      ka.out = scratch; ka.out_cs = ka.Co;
      ka.ks = op.ks; ka.kpart = (long long)B * V * ka.Co;
      CM_HIP(cm::launch_conv(ka, op.MB, op.NB, st));
      cm::CombineArgs cb{};
      cb.part = scratch; cb.S = op.ks; cb.stride = ka.kpart;
      cb.bias = ca.bias; cb.temb = ca.temb; cb.temb_stride = ca.temb_stride; cb.tidx = ca.tidx;
      cb.resid = ca.resid; cb.res_cs = ca.res_cs;
      cb.out = ca.out; cb.C = ka.Co; cb.V = V; cb.B = B;
      cb.nslots = p.ns_out; cb.stat_part = ca.stat_part; cb.stat_cnt = ca.stat_cnt;
      return run_combine(cb, m->ops, plan, p.carries, b0, st);
    }
    case CONV_UPS:
      // upsample conv: stage-once parity kernel with its own source tile / statistics slots
      if (route.form == FORM_F16) { ca.wfrag = op.d_wups16; ca.wpar_stride = op.wups16_stride; }
      else if (route.form != FORM_FP32) { ca.wfrag = op.d_wups_b6; ca.wpar_stride = op.wups_b6_stride; }
      ca.f16 = route.form;
      if (route.form == FORM_H2) {
        // default plan, inference-only handle: h2 with the sample's block exponent from the source tensor's slot statistics
        ca.wfrag = op.d_wups_h2; ca.h2_oscale = op.h2_oscale;
        ca.gp0 = slot_part(op.in0, p.ns0, b0); ca.gc0 = slot_cnt(op.in0, p.ns0, b0); ca.gns0 = p.ns0;
      }
      ca.bz = op.ups_tz; ca.by = op.ups_ty; ca.bx = op.ups_tx;
      ca.ntz = ca.Zs / ca.bz; ca.nty = ca.Ys / ca.by; ca.ntx = ca.Xs / ca.bx;
      CM_HIP(cm::launch_conv_ups(ca, op.ups_mbw, op.ups_planes, op.NB, st));
      break;
    case CONV_F16D:
      // reduced-precision plan: direct f16 kernel with its own tile geometry / statistics slots
      ca.bz = op.f16d_bz; ca.by = op.f16d_by; ca.bx = op.f16d_bx;
      ca.wfrag = op.d_w16d;
      if (ca.s2w) ca.s2w = op.d_w16d_skip;
      CM_HIP(cm::launch_conv_f16d(ca, op.f16d_mbw, st));
      break;
    case CONV_WINO: {
      const bool f16 = route.form == FORM_F16;
      ca.wfrag = f16 ? (train ? op.d_wwino16t : op.d_wwino16) : route.form == FORM_H2 ? op.d_wwino_h2 : route.form == FORM_FP32 ? op.d_wwino : op.d_wwino_b6;
      if (!f16) ca.f16 = route.form;
      if (route.form == FORM_H2) ca.h2_oscale = op.h2_oscale;
      // FIN_WINO: the GroupNorm of the input from the producers' slot partials, merged in the kernel's prologue
      if (ca.gn && op.gn_op >= 0 && plan.ops[op.gn_op].fin == FIN_WINO) {
        const Op &g = m->ops[op.gn_op]; const OpPlan &gp = plan.ops[op.gn_op];
        ca.gp0 = slot_part(g.g0, gp.ns0, b0); ca.gc0 = slot_cnt(g.g0, gp.ns0, b0); ca.gns0 = gp.ns0;
        if (g.g1) { ca.gp1 = slot_part(g.g1, gp.ns1, b0); ca.gc1 = slot_cnt(g.g1, gp.ns1, b0); ca.gns1 = gp.ns1; }
        ca.gs_gamma = g.gamma; ca.gs_beta = g.beta; ca.gs_groups = GN_GROUPS; ca.gs_eps = GN_EPS; ca.gn = nullptr;
      }
      CM_HIP(cm::launch_conv_wino(ca, f16, st));
      break;
    }
    case CONV_FIRST:
      if (le && op.ca.src0 == m->x8) ca.tz_first = le->tz_first;   // (a later loop step: the constant z tiles stay)
      CM_HIP(cm::launch_conv_first(ca, op.first_cin, op.d_wfirst, st));
      break;
    case CONV_FIN: {
      const ConvForm f = route.form;      // (launch_conv_fin's modes: 0 six bf16 terms, 1 f16, 2 three bf16 terms, 3 h2)
      ca.by = op.fin_by; ca.bx = op.fin_bx;
      ca.h2_oscale = op.h2_oscale;
      const bool ends = le && le->zo_end && op.ca.out == m->eps_cl;     // (a loop step: future planes only, the update in the tail)
      if (ends) { ca.zo_first = le->zo_first; ca.zo_end = le->zo_end; }
      CM_HIP(cm::launch_conv_fin(ca, f == FORM_F16 ? op.d_wfin16 : f == FORM_H2 ? op.d_wfin_h2 : op.d_wfin, f == FORM_F16 ? 1 : f == FORM_H2 ? 3 : f == FORM_B3 ? 2 : 0, st,
                                 ends && le->fuse ? le->step : nullptr, ends ? le->fuse : 0));
      break;
    }
    case CONV_SMALLN:
      CM_HIP(cm::launch_conv_smalln(ca, op.MB, op.d_wsmall, st));
      break;
    case CONV_1X1_F16:
      ca.wfrag = op.d_w1x1_16;
      CM_HIP(cm::launch_conv1x1_f16(ca, op.NB, st));
      break;
    case CONV_GENERIC:
      if (route.form == FORM_F16) { ca.wfrag = op.d_wfrag16; ca.wpar_stride = op.wpar_stride16; ca.f16 = 1; }   // f16 operands, fp32 accumulate
      CM_HIP(cm::launch_conv(ca, op.MB, op.NB, st));
      break;
  }
  return 0;
}

// The fused attention block `op` (plan entry `p`) for the plan.ctx.B samples from b0: the whole-sample launch where the plan takes it,
// else the (head, sample) launch and the head sum
int run_attn_block(const cm_model *m, const Op &op, const FwdPlan &plan, const OpPlan &p, hipStream_t st, int b0, int slab) {
  const std::vector<Op> &ops = m->ops; const int B = plan.ctx.B;
  const Op &gop = ops[op.ab_gn], &qop = ops[op.ab_qkv], &oop = ops[op.ab_outc];
  const size_t xoff = (size_t)b0 * op.S * op.E;
  if (p.attn_sample) {
    cm::AttnSampleArgs as{};
    as.x = op.ab_x->d + xoff; as.gamma = gop.gamma; as.beta = gop.beta;
    as.win_h2 = op.d_win_h2; as.b_in = qop.ca.bias; as.wout_h2 = op.d_wout_h2; as.b_out = oop.ca.bias;
    as.in_oscale = op.ab_in_oscale; as.out_oscale = op.ab_out_oscale;
    as.out = op.ab_out->d + xoff; as.B = B; as.S = op.S; as.nslots = p.ns_out; as.eps = GN_EPS;
    as.stat_part = slot_part(op.ab_out, p.ns_out, b0); as.stat_cnt = slot_cnt(op.ab_out, p.ns_out, b0);
    CM_HIP(cm::launch_attn_sample(as, st));
    return 0;
  }
  float *scratch = m->ks_scratch + (size_t)slab * m->ks_scratch_floats;
  cm::AttnBlockArgs aa{};
  aa.x = op.ab_x->d + xoff; aa.gamma = gop.gamma; aa.beta = gop.beta;
  aa.w_in = op.d_win; aa.b_in = qop.ca.bias; aa.w_out = op.d_wout;
  aa.part = scratch; aa.B = B; aa.S = op.S; aa.E = op.E; aa.heads = ATTN_HEADS; aa.groups = GN_GROUPS; aa.eps = GN_EPS;
  CM_HIP(cm::launch_attn_block(aa, st));
  cm::CombineArgs cb{};
  cb.part = scratch; cb.S = ATTN_HEADS; cb.stride = (long long)B * op.S * op.E;
  cb.bias = oop.ca.bias; cb.temb = nullptr; cb.tidx = m->tbuf;
  cb.resid = aa.x; cb.res_cs = op.E;
  cb.out = op.ab_out->d + xoff; cb.C = op.E; cb.V = op.S; cb.B = B;
  cb.nslots = p.ns_out; cb.stat_part = slot_part(op.ab_out, p.ns_out, b0); cb.stat_cnt = slot_cnt(op.ab_out, p.ns_out, b0);
  return run_combine(cb, ops, plan, p.carries, b0, st);
}

// Launch the op list as `plan` says, for plan.ctx.B samples starting at sample `b0` on stream `st`.
// Every sample-indexed pointer is offset by b0, so two disjoint sub-batches can run
// concurrently on two streams (`slab` selects the stream's K-split scratch region).
int run_ops(cm_model *m, const FwdPlan &plan, hipStream_t st, int b0 = 0, int slab = 0, const LoopEnds *le = nullptr) {
  const std::vector<Op> &ops = m->ops; const int B = plan.ctx.B;
  for (size_t oi = 0; oi < ops.size(); ++oi) {
    const Op &op = ops[oi]; const OpPlan &p = plan.ops[oi];
    if (!p.launch) continue;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (m->profile) {
      CM_HIP(hipEventCreate(&e0));
      CM_HIP(hipEventCreate(&e1));
      CM_HIP(hipEventRecord(e0, st));
    }
    static const bool sync_ops = cm::diag_env("CM_SYNC_OPS") != nullptr;   // debugging: name every op and drain the device before it
    if (sync_ops) {
      const hipError_t e = hipDeviceSynchronize();
      fprintf(stderr, "[cm] forward reaches op %zu %s (%s)\n", oi, op.label.c_str(), hipGetErrorString(e));
      fflush(stderr);
    }
    switch (op.kind) {
      case OP_CONV:
        if (run_conv(m, op, plan, p, st, b0, slab, le)) return 1;
        break;
      case OP_STATS:
        CM_HIP(cm::launch_chan_stats(op.act->d + (size_t)b0 * op.act->V() * op.act->C, B, op.act->V(), op.act->C, p.ns_out,
                                     slot_part(op.act, p.ns_out, b0), slot_cnt(op.act, p.ns_out, b0), st));
        break;
      case OP_GNFIN:                     // FIN_ALONE (every other disposition launches nothing here)
        if (run_gnfin(op, p, B, st, b0)) return 1;
        break;
      case OP_ATTN: {
        // reduced-precision plan, inference: QK^T and PV on f16 matrix-core operands (the fp32 plan and every training
        // forward keep the exact fp32 kernel)
        const bool f16 = plan.ctx.precision == CM_PRECISION_F16 && !plan.ctx.train_fwd && op.E / ATTN_HEADS == 32 && !cm::diag_env("CM_NO_ATTN_F16");
        CM_HIP((f16 ? cm::launch_attn_core_f16 : cm::launch_attn_core)(op.qkv + (size_t)b0 * op.S * 3 * op.E, op.aout + (size_t)b0 * op.S * op.E,
                                                                      B, op.S, op.E, ATTN_HEADS, st));
        break;
      }
      case OP_ATTNBLK:
        if (run_attn_block(m, op, plan, p, st, b0, slab)) return 1;
        break;
    }
    if (m->profile) {
      CM_HIP(hipEventRecord(e1, st));
      m->prof_events[slab & 3].push_back({(int)oi, {e0, e1}});
    }
  }
  return 0;
}

int prof_begin(cm_model *m, hipStream_t st) {
  if (!m->profile) return 0;
  for (int i = 0; i < K_NCLASS; ++i) { m->prof_ms[i] = 0; m->prof_n[i] = 0; m->prof_union_ms[i] = 0; }
  for (Op &op : m->ops) { op.prof_ms = 0; op.prof_n = 0; }
  if (!m->prof_base) CM_HIP(hipEventCreate(&m->prof_base));
  CM_HIP(hipEventRecord(m->prof_base, st));
  return 0;
}

// Per-launch durations (summed per op and per class) and, per class, the length of the UNION of the launch intervals over
// all batch lanes: with two lanes the launches of one class overlap each other and other classes, so "class time" is the
// time during which at least one launch of the class was running (all offsets against prof_base).
int prof_collect(cm_model *m, hipStream_t st) {
  if (!m->profile) return 0;
  CM_HIP(hipDeviceSynchronize()); (void)st;
  m->prof_B = m->plan.ctx.B;
  std::vector<std::pair<float, float>> iv[K_NCLASS];
  for (int ln = 0; ln < 4; ++ln) {
    for (auto &pe : m->prof_events[ln]) {
      float t0 = 0, t1 = 0;
      CM_HIP(hipEventElapsedTime(&t0, m->prof_base, pe.second.first));
      CM_HIP(hipEventElapsedTime(&t1, m->prof_base, pe.second.second));
      const float ms = t1 - t0;
      Op &op = m->ops[pe.first];
      op.prof_ms += ms;
      op.prof_n += 1;
      m->prof_ms[op.cls] += ms;
      m->prof_n[op.cls] += 1;
      iv[op.cls].push_back({t0, t1});
      hipEventDestroy(pe.second.first);
      hipEventDestroy(pe.second.second);
    }
    m->prof_events[ln].clear();
  }
  for (int c = 0; c < K_NCLASS; ++c) {
    std::sort(iv[c].begin(), iv[c].end());
    float total = 0, lo = 0, hi = -1;
    for (auto &x : iv[c]) {
      if (hi < lo || x.first > hi) { if (hi >= lo) total += hi - lo; lo = x.first; hi = x.second; }
      else hi = std::max(hi, x.second);
    }
    if (hi >= lo) total += hi - lo;
    m->prof_union_ms[c] = total;
  }
  return 0;
}

// Makes `dev` current for the duration of one C-ABI call and restores the caller's device on return.
struct DevGuard {
  int prev = -1, cur = -1;
  explicit DevGuard(int dev) : cur(dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) hipSetDevice(dev);
  }
  ~DevGuard() {
    if (prev >= 0 && prev != cur) hipSetDevice(prev);
  }
  DevGuard(const DevGuard &) = delete;
  DevGuard &operator=(const DevGuard &) = delete;
};

int check_ready(cm_model *m, int B) {
  if (!m) return fail("null model handle");
  if (!m->finalized) return fail("cm_model_finalize has not been called");
  if (B < 1 || B > m->cfg.max_batch) return fail("batch %d outside [1, max_batch=%d]", B, m->cfg.max_batch);
  return 0;
}

// Entry points plan on the calling thread, before anything is enqueued; their own plan goes into cm_model::plan, which nothing else writes.
int make_plan(const cm_model *m, bool train_fwd, int B, FwdPlan *plan) {
  *plan = plan_forward(m->ops, FwdCtx{m->precision, train_fwd, m->h2_stale, B, train_fwd && m->train_autocast});
  return plan->err.empty() ? 0 : fail("%s", plan->err.c_str());
}

// A debug hook launches ONE, possibly modified, conv against what the last forward left: `plan` becomes that forward's plan at batch B in the
// inference context, entry `index` planned again for `op` (`src_slots` > 0: its source statistics, just recomputed in that many slots).  Where
// that forward left the GroupNorm to this conv's slot merge and this launch cannot merge, it is finalised here.
int plan_debug_conv(const cm_model *m, const Op &op, int index, int B, int src_slots, hipStream_t st, FwdPlan *plan) {
  if (!m->plan.err.empty() || m->plan.ops.size() != m->ops.size()) return fail("no forward has run on this handle");
  *plan = m->plan; plan->ctx = FwdCtx{m->precision, false, m->h2_stale, B};
  OpPlan &p = plan->ops[index], &gp = plan->ops[std::max(op.gn_op, 0)];
  p.carries = -1;                    // a hook's second pass is the plain combine: no other op's scale / shift rows are touched
  if (const std::string err = plan_conv(op, plan->ctx, src_slots > 0 ? src_slots : p.ns0, &p); !err.empty()) return fail("%s", err.c_str());
  if (!op.ca.gn || op.gn_op < 0 || gp.fin != FIN_WINO || wino_merges(op, p.route, B)) return 0;
  gp.fin = FIN_ALONE;
  return run_gnfin(m->ops[op.gn_op], gp, B, st, 0);
}

// torch.linspace / cumprod semantics of forward.py:15-27 (see oracle/unet_numpy.py:
// fp32 step, symmetric fill, fused multiply-add; cumprod accumulated in double).
void build_schedule(cm_schedule *s, int T, float scale, float beta_start, float beta_end) {
  s->T = T;
  for (auto &t : s->tab) t.assign((size_t)T, 0.f);
  const float start = (float)((double)scale * (double)beta_start), end = (float)((double)scale * (double)beta_end);
  const double step = (double)(float)(((double)end - (double)start) / (double)(T - 1));
  double acc = 1.0;
  for (int i = 0; i < T; ++i) {
    const double b = (i < T / 2) ? (double)start + step * i : (double)end - step * (T - 1 - i);
    const float beta = (float)b;
    const float alpha = 1.0f - beta;
    acc *= (double)alpha;
    const float abar = (float)acc;
    s->tab[CM_TAB_BETA][i] = beta;
    s->tab[CM_TAB_ALPHA][i] = alpha;
    s->tab[CM_TAB_ALPHA_BAR][i] = abar;
    s->tab[CM_TAB_SQRT_ALPHA_BAR][i] = sqrtf(abar);
    s->tab[CM_TAB_ONE_BY_SQRT_ALPHA][i] = 1.0f / sqrtf(alpha);
    s->tab[CM_TAB_SQRT_ONE_MINUS_ALPHA_BAR][i] = sqrtf(1.0f - abar);
  }
}

// torch.linspace(start, end, n)[i] in fp32: symmetric fill around the midpoint, one fused multiply-add
// per element (the same restatement as the beta schedule; oracle/unet_numpy.py linspace_f32)
float linspace_f32(float start, float end, int n, int i) {
  if (n == 1) return start;
  const double step = (double)(float)(((double)end - (double)start) / (double)(n - 1));
  const double b = (i < n / 2) ? (double)start + step * i : (double)end - step * (n - 1 - i);
  return (float)b;
}

std::vector<int> visit_order(const cm_schedule *s, const cm_sample_opts *o) {
  std::vector<int> v;
  if (o->sampler == CM_SAMPLER_FM_EULER) {
    // time index per Euler step: (t * TIME_MAX_POS).clamp(0, TIME_MAX_POS - 1).long(), flow_matching.py:214
    const int n = std::max(1, o->fm_steps), tmp = std::max(1, o->fm_time_max_pos);
    for (int i = 0; i < n; ++i) {
      float x = linspace_f32(0.f, 1.f, n, i) * (float)tmp;
      x = std::min(std::max(x, 0.f), (float)(tmp - 1));
      v.push_back((int)x);
    }
  } else if (o->sampler == CM_SAMPLER_DDIM) {
    const int d = std::max(1, o->ddim_divider);
    std::vector<int> taus;
    for (int t = 0; t < s->T - 1; t += d) taus.push_back(t);  // np.arange(0, T-1, divider), ddpm.py:326
    v.assign(taus.rbegin(), taus.rend());
  } else {
    for (int t = s->T - 1; t >= 0; --t) v.push_back(t);       // reversed(range(T)), ddpm.py:214
  }
  if (o->first_steps > 0 && (size_t)o->first_steps < v.size()) v.resize((size_t)o->first_steps);
  return v;
}

}  // namespace

#include "cm_dit_host.inc"

namespace {
// entry points of the UNet plan that a DiT handle does not have
int refuse_dit(const cm_model *m, const char *what) {
  return fail("%s: not available on a %s handle, only on the UNet backbone", what,
              m->dit->full ? "FM-DiT (DiT2D)" : "DDPM-DiT (DiT4D_V4)");
}
}  // namespace
#define CM_NOT_DIT(m, what) do { if ((m) && (m)->dit) return refuse_dit(m, what); } while (0)

// ================================================================================
// C ABI
// ================================================================================
extern "C" {

const char *cm_last_error(void) { return g_err.c_str(); }
int cm_abi_version(void) { return CM_ABI_VERSION; }

int cm_device_count(int *count) {
  if (!count) return fail("null argument");
  CM_HIP(hipGetDeviceCount(count));
  return 0;
}

int cm_malloc(int device, void **d_ptr, size_t bytes) {
  if (!d_ptr) return fail("null argument");
  DevGuard g(device);
  CM_HIP(hipMalloc(d_ptr, bytes ? bytes : 4));
  return 0;
}
int cm_free(int device, void *d_ptr) {
  DevGuard g(device);
  CM_HIP(hipFree(d_ptr));
  return 0;
}
int cm_memcpy_h2d(int device, void *d_dst, const void *h_src, size_t bytes) {
  DevGuard g(device);
  CM_HIP(hipMemcpy(d_dst, h_src, bytes, hipMemcpyHostToDevice));
  return 0;
}
int cm_memcpy_d2h(int device, void *h_dst, const void *d_src, size_t bytes) {
  DevGuard g(device);
  CM_HIP(hipMemcpy(h_dst, d_src, bytes, hipMemcpyDeviceToHost));
  return 0;
}
int cm_memcpy_d2d(int device, void *d_dst, const void *d_src, size_t bytes) {
  DevGuard g(device);
  CM_HIP(hipMemcpy(d_dst, d_src, bytes, hipMemcpyDeviceToDevice));
  return 0;
}
int cm_device_synchronize(int device) {
  DevGuard g(device);
  CM_HIP(hipDeviceSynchronize());
  return 0;
}

int cm_model_create(const cm_unet_config *cfg, cm_model **out) {
  if (!cfg || !out) return fail("null argument");
  if (cfg->n_levels < 1 || cfg->n_levels > CM_MAX_LEVELS) return fail("n_levels %d out of range", cfg->n_levels);
  if (cfg->base_channels < 8 || cfg->base_channels % 8) return fail("base_channels must be a positive multiple of 8");
  if (cfg->in_channels < 1 || cfg->in_channels > 8 || cfg->out_channels < 1 || cfg->out_channels > 8)
    return fail("in/out channels must be in [1,8]");
  if (cfg->max_batch < 1) return fail("max_batch must be >= 1");
  if (cfg->num_res_blocks < 1) return fail("num_res_blocks must be >= 1");
  if ((cfg->base_channels / 2) < 2) return fail("base_channels too small for the sinusoidal table");
  // device < 0: host-only handle -- the state_dict plan (names, shapes, set / get) without a GPU
  // (checkpoint tooling, the sanitizer self-test); cm_model_finalize and everything after it need a device
  if (cfg->device >= 0) {
    int ndev = 0;
    CM_HIP(hipGetDeviceCount(&ndev));
    if (cfg->device >= ndev) return fail("device %d not available (%d devices)", cfg->device, ndev);
  }
  auto m = std::make_unique<cm_model>();
  m->cfg = *cfg;
  m->device = cfg->device;
  for (int l = 0; l < cfg->n_levels; ++l)
    if (cfg->channel_mult[l] < 1 || (cfg->base_channels * cfg->channel_mult[l]) % (GN_GROUPS) != 0)
      return fail("channel_mult[%d] invalid", l);
  build_plan(m.get());
  if (m->device < 0) { *out = m.release(); return 0; }
  DevGuard g(m->device);
  CM_HIP(hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking));
  for (int i = 1; i < 4; ++i) {
    CM_HIP(hipStreamCreateWithFlags(&m->lane_stream[i], hipStreamNonBlocking));
    CM_HIP(hipEventCreateWithFlags(&m->ev_join[i], hipEventDisableTiming));
  }
  CM_HIP(hipEventCreateWithFlags(&m->ev_fork, hipEventDisableTiming));
  *out = m.release();
  return 0;
}

int cm_model_destroy(cm_model *m) {
  if (!m) return 0;
  delete m->dit;
  if (m->device < 0) {
    for (void *p : m->allocs) free(p);
    delete m;
    return 0;
  }
  DevGuard g(m->device);
  hipDeviceSynchronize();
  for (void *p : m->allocs) hipFree(p);
  if (m->stream) hipStreamDestroy(m->stream);
  for (int i = 1; i < 4; ++i) {
    if (m->lane_stream[i]) hipStreamDestroy(m->lane_stream[i]);
    if (m->ev_join[i]) hipEventDestroy(m->ev_join[i]);
  }
  if (m->ev_fork) hipEventDestroy(m->ev_fork);
  if (m->prof_base) hipEventDestroy(m->prof_base);
  if (m->train) cm_free_train_state(m->train);
  delete m;
  return 0;
}

int cm_model_num_params(const cm_model *m, int32_t *count) {
  if (!m || !count) return fail("null argument");
  *count = (int32_t)m->params.size();
  return 0;
}

int cm_model_param_info(const cm_model *m, int32_t index, const char **name, int64_t shape[5], int32_t *ndim) {
  if (!m || index < 0 || index >= (int)m->params.size()) return fail("parameter index out of range");
  const Param &p = m->params[index];
  if (name) *name = p.name.c_str();
  if (ndim) *ndim = (int32_t)p.shape.size();
  if (shape)
    for (size_t i = 0; i < 5; ++i) shape[i] = i < p.shape.size() ? p.shape[i] : 1;
  return 0;
}

int cm_model_set_param(cm_model *m, const char *name, const float *h_data, int64_t numel) {
  if (!m || !name || !h_data) return fail("null argument");
  auto it = m->pindex.find(name);
  if (it == m->pindex.end()) return fail("unexpected key in state_dict: %s", name);
  Param &p = m->params[it->second];
  if (numel != p.numel()) return fail("size mismatch for %s: got %lld elements, expected %lld", name, (long long)numel, (long long)p.numel());
  if (m->finalized) return fail("model already finalized; create a new handle to load other weights");
  std::memcpy(p.host.data(), h_data, (size_t)numel * sizeof(float));
  p.set = true;
  return 0;
}

int cm_model_get_param(const cm_model *m, const char *name, float *h_data, int64_t numel) {
  if (!m || !name || !h_data) return fail("null argument");
  auto it = m->pindex.find(name);
  if (it == m->pindex.end()) return fail("unknown parameter %s", name);
  const Param &p = m->params[it->second];
  if (numel != p.numel()) return fail("size mismatch for %s", name);
  std::memcpy(h_data, p.host.data(), (size_t)numel * sizeof(float));
  return 0;
}

int cm_model_set_precision(cm_model *m, int32_t precision) {
  if (!m) return fail("null model handle");
  if (m->finalized) return fail("precision must be chosen before cm_model_finalize");
  if (precision != CM_PRECISION_F32 && precision != CM_PRECISION_F16 && precision != CM_PRECISION_F32R && precision != CM_PRECISION_F32X &&
      precision != CM_PRECISION_F16A)
    return fail("unknown precision %d", precision);
  if (precision == CM_PRECISION_F16A && !(m->dit && m->dit->full))
    return fail("CM_PRECISION_F16A (f16 operands, attention included) is the reduced-precision plan of FM-DiT (DiT2D) handles: a %s handle "
                "takes CM_PRECISION_F16", m->dit ? "DDPM-DiT (DiT4D_V4)" : "UNet");
  if (m->dit && m->dit->full && precision == CM_PRECISION_F16)
    return fail("CM_PRECISION_F16 is the plan of UNet and DDPM-DiT handles (fp32 attention): an FM-DiT (DiT2D) handle takes CM_PRECISION_F32 "
                "or CM_PRECISION_F16A, whose attention products take f16 operands as well");
  if (m->dit && m->dit->full && precision != CM_PRECISION_F32 && precision != CM_PRECISION_F16A)
    return fail("CM_PRECISION_F32R and CM_PRECISION_F32X are split forms of the UNet's convs: an FM-DiT (DiT2D) handle takes "
                "CM_PRECISION_F32 or CM_PRECISION_F16A");
  if (m->dit && (precision == CM_PRECISION_F32R || precision == CM_PRECISION_F32X))
    return fail("CM_PRECISION_F32R and CM_PRECISION_F32X are split forms of the UNet's convs: a DDPM-DiT (DiT4D_V4) handle takes "
                "CM_PRECISION_F32 or CM_PRECISION_F16");
  m->precision = precision;
  return 0;
}

int cm_model_finalize(cm_model *m) {
  if (!m) return fail("null model handle");
  if (m->finalized) return 0;
  if (m->device < 0) return fail("host-only handle (device < 0) cannot be finalized: there is no CPU path");
  for (auto &p : m->params)
    if (!p.set) return fail("missing key in state_dict: %s", p.name.c_str());
  if (m->dit) return dit_finalize(m);
  DevGuard g(m->device);
  const cm_unet_config &c = m->cfg;
  const size_t B = (size_t)c.max_batch;
  if (dev_alloc(m, (void **)&m->tbuf, B * sizeof(long long))) return 1;
  CM_HIP(hipMemset(m->tbuf, 0, B * sizeof(long long)));
  if (build_ops(m)) return 1;
  for (Op &op : m->ops)
    if (op.kind == OP_CONV && resolve_conv(m, op)) return 1;
  if (plan_h16(m)) return 1;
  if (build_time_table(m)) return 1;
  const size_t per = (size_t)m->per_sample();
  const size_t per_past = (size_t)c.in_channels * c.rows * c.cols * c.past_len;
  if (dev_alloc(m, (void **)&m->xstate, B * per * sizeof(float))) return 1;
  if (dev_alloc(m, (void **)&m->dropmask, B * (size_t)m->nproj * sizeof(float))) return 1;
  if (dev_alloc(m, (void **)&m->mse_partial, 64 * sizeof(float))) return 1;
  if (dev_alloc(m, (void **)&m->mse_loss, sizeof(float))) return 1;
  if (dev_alloc(m, (void **)&m->stage_fut, B * per * sizeof(float))) return 1;
  if (dev_alloc(m, (void **)&m->stage_out, B * per * sizeof(float))) return 1;
  if (dev_alloc(m, (void **)&m->stage_past, B * per_past * sizeof(float))) return 1;
  CM_HIP(hipDeviceSynchronize());
  m->finalized = true;
  return 0;
}

int cm_unet_forward(cm_model *m, const float *d_future, const int64_t *d_t, const float *d_past, float *d_out,
                    int32_t B, void *stream) {
  if (check_ready(m, B)) return 1;
  if (m->h2_stale && refresh_h2(m)) return 1;
  if (!d_future || !d_t || !d_past || !d_out) return fail("null tensor argument");
  DevGuard g(m->device);
  hipStream_t st = stream ? (hipStream_t)stream : m->stream;
  const cm_unet_config &c = m->cfg;
  if (make_plan(m, false, B, &m->plan) || prof_begin(m, st)) return 1;
  CM_HIP(hipMemcpyAsync(m->tbuf, d_t, (size_t)B * sizeof(long long), hipMemcpyDeviceToDevice, st));
  CM_HIP(cm::launch_assemble_input(d_past, d_future, m->x8, B, c.in_channels, c.rows, c.cols, c.past_len, c.future_len, 3, st));
  if (denoise(m, m->plan, st, 0, 0)) return 1;
  CM_HIP(cm::launch_extract_output(m->eps_cl, 8, d_out, B, c.out_channels, c.rows, c.cols, c.past_len, c.future_len, st));
  return prof_collect(m, st);
}

int cm_unet_forward_host(cm_model *m, const float *h_future, const int64_t *h_t, const float *h_past, float *h_out,
                         int32_t B) {
  if (check_ready(m, B)) return 1;
  if (!h_future || !h_t || !h_past || !h_out) return fail("null tensor argument");
  DevGuard g(m->device);
  const cm_unet_config &c = m->cfg;
  for (int i = 0; i < B; ++i)
    if (h_t[i] < 0 || h_t[i] >= TIME_ROWS) return fail("timestep %lld outside [0,%d)", (long long)h_t[i], TIME_ROWS);
  const size_t per = (size_t)m->per_sample();
  const size_t per_past = (size_t)c.in_channels * c.rows * c.cols * c.past_len;
  CM_HIP(hipMemcpy(m->stage_fut, h_future, B * per * sizeof(float), hipMemcpyHostToDevice));
  CM_HIP(hipMemcpy(m->stage_past, h_past, B * per_past * sizeof(float), hipMemcpyHostToDevice));
  long long *dt = nullptr;
  CM_HIP(hipMalloc((void **)&dt, (size_t)B * sizeof(long long)));
  hipError_t e = hipMemcpy(dt, h_t, (size_t)B * sizeof(long long), hipMemcpyHostToDevice);
  int rc = (e != hipSuccess) ? fail("hipMemcpy t failed") : cm_unet_forward(m, m->stage_fut, (const int64_t *)dt, m->stage_past, m->stage_out, B, nullptr);
  if (!rc) {
    e = hipStreamSynchronize(m->stream);
    if (e != hipSuccess) rc = fail("forward failed: %s", hipGetErrorString(e));
  }
  hipFree(dt);
  if (rc) return rc;
  CM_HIP(hipMemcpy(h_out, m->stage_out, B * per * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}

int cm_model_dropout_width(const cm_model *m, int32_t *width) {
  CM_NOT_DIT(m, "cm_model_dropout_width");
  if (!m || !width) return fail("null argument");
  if (!m->finalized) return fail("model not finalized");
  *width = m->nproj;
  return 0;
}

int cm_unet_forward_train(cm_model *m, const float *d_future, const int64_t *d_t, const float *d_past,
                          const float *d_dropmask, float p, uint64_t seed, int64_t sample_id_base, float *d_out,
                          int32_t B, void *stream) {
  CM_NOT_DIT(m, "cm_unet_forward_train");
  if (check_ready(m, B)) return 1;
  if (!d_future || !d_t || !d_past || !d_out) return fail("null tensor argument");
  if (!(p >= 0.f && p < 1.f)) return fail("dropout rate %g outside [0,1)", p);
  DevGuard g(m->device);
  hipStream_t st = stream ? (hipStream_t)stream : m->stream;
  const cm_unet_config &c = m->cfg;
  if (make_plan(m, true, B, &m->plan)) return 1;
  if (d_dropmask)
    CM_HIP(hipMemcpyAsync(m->dropmask, d_dropmask, (size_t)B * m->nproj * sizeof(float), hipMemcpyDeviceToDevice, st));
  else
    CM_HIP(cm::launch_dropout_mask(m->dropmask, B, m->nproj, p, seed, sample_id_base, 0, st));
  CM_HIP(hipMemcpyAsync(m->tbuf, d_t, (size_t)B * sizeof(long long), hipMemcpyDeviceToDevice, st));
  CM_HIP(cm::launch_assemble_input(d_past, d_future, m->x8, B, c.in_channels, c.rows, c.cols, c.past_len, c.future_len, 3, st));
  if (run_ops(m, m->plan, st)) return 1;
  CM_HIP(cm::launch_extract_output(m->eps_cl, 8, d_out, B, c.out_channels, c.rows, c.cols, c.past_len, c.future_len, st));
  return 0;
}

int cm_mse_loss(cm_model *m, const float *d_pred, const float *d_target, int64_t n, float *h_loss, void *stream) {
  CM_NOT_DIT(m, "cm_mse_loss");
  if (!m || !d_pred || !d_target || !h_loss || n < 1) return fail("bad argument");
  if (!m->finalized) return fail("model not finalized");
  DevGuard g(m->device);
  hipStream_t st = stream ? (hipStream_t)stream : m->stream;
  CM_HIP(cm::launch_mse_loss(d_pred, d_target, n, m->mse_partial, m->mse_loss, st));
  CM_HIP(hipMemcpyAsync(h_loss, m->mse_loss, sizeof(float), hipMemcpyDeviceToHost, st));
  CM_HIP(hipStreamSynchronize(st));
  return 0;
}

int cm_debug_dit_attn(cm_model *m, const float *h_qkv, float *h_out, int32_t B) {
  if (!m || !h_qkv || !h_out) return fail("null argument");
  if (!m->dit || !m->dit->full)
    return fail("cm_debug_dit_attn: a %s handle has no full-attention launch; this entry point takes FM-DiT (DiT2D) handles only",
                m->dit ? "DDPM-DiT (DiT4D_V4)" : "UNet");
  if (!m->finalized) return fail("cm_debug_dit_attn: model not finalized");
  return dit_debug_attn(m, h_qkv, h_out, B);
}

int cm_debug_activation(cm_model *m, const char *name, float *h_out, int64_t capacity, int64_t shape[5]) {
  if (!m || !name || !h_out) return fail("null argument");
  if (!m->finalized) return fail("model not finalized");
  if (m->dit) return dit_debug_activation(m, name, h_out, capacity, shape);
  auto it = m->act_by_name.find(name);
  if (it == m->act_by_name.end()) return fail("no activation named %s", name);
  const Act *a = it->second;
  DevGuard g(m->device);
  const int B = m->cfg.max_batch;
  const int C = a->C;
  const int64_t n = (int64_t)B * C * a->V();
  if (capacity < n) return fail("capacity %lld < %lld", (long long)capacity, (long long)n);
  if (a->h16) {
    // f16 tensor of the reduced-precision plan: fetched as stored, converted and re-laid [B,C,H,W,L] on the host (test hook)
    std::vector<uint16_t> raw((size_t)n);
    CM_HIP(hipStreamSynchronize(m->stream));
    CM_HIP(hipMemcpy(raw.data(), a->d, (size_t)n * sizeof(uint16_t), hipMemcpyDeviceToHost));
    for (int b = 0; b < B; ++b)
      for (int z = 0; z < a->Z; ++z)
        for (int y = 0; y < a->Y; ++y)
          for (int x = 0; x < a->X; ++x)
            for (int c = 0; c < C; ++c)
              h_out[((((size_t)b * C + c) * a->Y + y) * a->X + x) * a->Z + z] =
                  f16_bits_to_f32(raw[((((size_t)b * a->Z + z) * a->Y + y) * a->X + x) * C + c]);
    if (shape) { shape[0] = B; shape[1] = C; shape[2] = a->Y; shape[3] = a->X; shape[4] = a->Z; }
    return 0;
  }
  float *tmp = nullptr;
  CM_HIP(hipMalloc((void **)&tmp, (size_t)n * sizeof(float)));
  hipError_t e = cm::launch_cl_to_ref(a->d, a->C, tmp, B, C, a->Z, a->Y, a->X, m->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(m->stream);
  if (e == hipSuccess) e = hipMemcpy(h_out, tmp, (size_t)n * sizeof(float), hipMemcpyDeviceToHost);
  hipFree(tmp);
  if (e != hipSuccess) return fail("debug copy failed: %s", hipGetErrorString(e));
  if (shape) { shape[0] = B; shape[1] = C; shape[2] = a->Y; shape[3] = a->X; shape[4] = a->Z; }
  return 0;
}

// ---- schedule -----------------------------------------------------------------
int cm_schedule_create(int32_t timesteps, float scale, float beta_start, float beta_end, int32_t device, cm_schedule **out) {
  if (!out) return fail("null argument");
  if (timesteps < 2) return fail("timesteps must be >= 2");
  auto s = std::make_unique<cm_schedule>();
  s->device = device;
  build_schedule(s.get(), timesteps, scale, beta_start, beta_end);
  if (device >= 0) {
    DevGuard g(device);
    CM_HIP(hipMalloc((void **)&s->d_sab, (size_t)timesteps * sizeof(float)));
    CM_HIP(hipMalloc((void **)&s->d_s1m, (size_t)timesteps * sizeof(float)));
    CM_HIP(hipMemcpy(s->d_sab, s->tab[CM_TAB_SQRT_ALPHA_BAR].data(), (size_t)timesteps * sizeof(float), hipMemcpyHostToDevice));
    CM_HIP(hipMemcpy(s->d_s1m, s->tab[CM_TAB_SQRT_ONE_MINUS_ALPHA_BAR].data(), (size_t)timesteps * sizeof(float), hipMemcpyHostToDevice));
  }
  *out = s.release();
  return 0;
}

int cm_schedule_destroy(cm_schedule *s) {
  if (!s) return 0;
  if (s->device >= 0) {
    DevGuard g(s->device);
    if (s->d_sab) hipFree(s->d_sab);
    if (s->d_s1m) hipFree(s->d_s1m);
  }
  delete s;
  return 0;
}

int cm_schedule_table(const cm_schedule *s, int32_t which, float *h_out, int32_t capacity) {
  if (!s || !h_out) return fail("null argument");
  if (which < 0 || which > 5) return fail("table id %d out of range", which);
  if (capacity < s->T) return fail("capacity %d < timesteps %d", capacity, s->T);
  std::memcpy(h_out, s->tab[which].data(), (size_t)s->T * sizeof(float));
  return 0;
}

int cm_q_sample(const cm_schedule *s, const float *d_x0, const int64_t *d_t, const float *d_eps, float *d_xt, int32_t B,
                int64_t per_sample, void *stream) {
  if (!s || !d_x0 || !d_t || !d_eps || !d_xt) return fail("null argument");
  if (s->device < 0) return fail("schedule was created host-only (device < 0)");
  DevGuard g(s->device);
  CM_HIP(cm::launch_q_sample(d_x0, (const long long *)d_t, d_eps, s->d_sab, s->d_s1m, d_xt, B, per_sample, (hipStream_t)stream));
  return 0;
}

static void ddpm_coeffs(const cm_schedule *s, int t, float *cx, float *ce, float *cn) {
  const float beta = s->tab[CM_TAB_BETA][t];
  const float c1 = s->tab[CM_TAB_ONE_BY_SQRT_ALPHA][t];
  const float s1m = s->tab[CM_TAB_SQRT_ONE_MINUS_ALPHA_BAR][t];
  *cx = c1;
  *ce = -c1 * (beta / s1m);
  *cn = sqrtf(beta);
}

int cm_ddpm_step(const cm_schedule *s, const float *d_eps, float *d_x, int32_t t, const float *d_noise, uint64_t seed,
                 int64_t sample_id_base, int32_t B, int64_t per_sample, void *stream) {
  if (!s || !d_eps || !d_x) return fail("null argument");
  if (t < 0 || t >= s->T) return fail("timestep %d outside [0,%d)", t, s->T);
  if (s->device < 0) return fail("schedule was created host-only (device < 0)");
  DevGuard g(s->device);
  // eps arrives in reference layout here: express it as a degenerate channels-last
  // tensor with C=1 (cs = 1, P = 0, H = W = 1, F = per_sample).
  cm::StepArgs a{};
  a.x = d_x; a.eps_cl = d_eps; a.cs = 1; a.x8 = nullptr; a.noise = d_noise; a.hist = nullptr;
  a.B = B; a.C = 1; a.H = 1; a.W = 1; a.P = 0; a.F = (int)per_sample;
  ddpm_coeffs(s, t, &a.c_x, &a.c_eps, &a.c_noise);
  a.guid = 0.f; a.seed = seed; a.sample_id_base = sample_id_base; a.step = t; a.draw = t > 0;
  CM_HIP(cm::launch_sampler_step(a, (hipStream_t)stream));
  return 0;
}

int cm_sample_num_steps(const cm_schedule *s, const cm_sample_opts *opts, int32_t *nsteps) {
  if (!s || !opts || !nsteps) return fail("null argument");
  *nsteps = (int32_t)visit_order(s, opts).size();
  return 0;
}

int cm_sample_loop(cm_model *m, const cm_schedule *s, const float *d_past, const float *d_xT, const float *d_noise,
                   const cm_sample_opts *opts, float *d_out, float *d_history, int32_t B, void *stream) {
  if (check_ready(m, B)) return 1;
  if (m->h2_stale && refresh_h2(m)) return 1;
  if (!s || !d_past || !opts || !d_out) return fail("null argument");
  if (s->T > TIME_ROWS) return fail("timesteps %d exceed the %d-row time-embedding table (embeddings.py:7)", s->T, TIME_ROWS);
  if (opts->sampler == CM_SAMPLER_FM_EULER && (opts->fm_steps < 1 || opts->fm_time_max_pos < 1 || opts->fm_time_max_pos > TIME_ROWS))
    return fail("flow-matching sampler needs fm_steps >= 1 and 1 <= fm_time_max_pos <= %d", TIME_ROWS);
  DevGuard g(m->device);
  hipStream_t st = stream ? (hipStream_t)stream : m->stream;
  const cm_unet_config &c = m->cfg;
  const size_t per = (size_t)m->per_sample();
  const std::vector<int> order = visit_order(s, opts);
  // mass_preservation guidance runs in the DDPM loop only (ddpm.py:227-229; _generate_ddim and flow matching ignore it)
  const bool mass = opts->guidance == CM_GUIDANCE_MASS_PRESERVATION && opts->sampler == CM_SAMPLER_DDPM;
  if (mass && c.in_channels < 3) return fail("mass_preservation guidance needs >= 3 channels (r, u, v), model has %d", c.in_channels);
  if (mass && !m->mass_q && dev_alloc(m, (void **)&m->mass_q, (size_t)c.max_batch * 3 * c.rows * c.cols * c.future_len * sizeof(float)))
    return 1;
  if (prof_begin(m, st)) return 1;
  // x_T: injected or drawn on device (ddpm.py:211,242)
  if (d_xT) CM_HIP(hipMemcpyAsync(m->xstate, d_xT, B * per * sizeof(float), hipMemcpyDeviceToDevice, st));
  else CM_HIP(cm::launch_randn(m->xstate, B, (long long)per, opts->seed, opts->sample_id_base, 0x7fffffff, st));
  if (d_history) CM_HIP(hipMemcpyAsync(d_history, m->xstate, B * per * sizeof(float), hipMemcpyDeviceToDevice, st));
  CM_HIP(cm::launch_assemble_input(d_past, m->xstate, m->x8, B, c.in_channels, c.rows, c.cols, c.past_len, c.future_len, 3, st));

  // DDIM carries the schedule values of the previously visited step (ddpm.py:245-248)
  const int last = s->T - 1;
  float beta_t = s->tab[CM_TAB_BETA][last], sab_t = s->tab[CM_TAB_SQRT_ALPHA_BAR][last],
        s1m_t = s->tab[CM_TAB_SQRT_ONE_MINUS_ALPHA_BAR][last];
  // Batch lanes (CM_LANES, default 2): the chains are independent, so the batch is cut in halves that run the whole step
  // sequence on separate streams, each enqueued by its own host thread, with bit-identical results; the ramp-up / tail and the
  // launch gaps of one lane are filled by the other lane's workgroups (-4.5 % per step at B = 64).  A profiled call keeps the
  // lanes: its per-class time is the union of the launch intervals over both lanes (prof_collect).
  static const int want_lanes = getenv("CM_LANES") ? atoi(getenv("CM_LANES")) : 2;
  int lanes = std::max(1, std::min(4, want_lanes));
  if (B < 8 * lanes || stream || opts->use_graph) lanes = 1;
  // a profiled call runs ONE lane unless CM_PROFILE_LANES is set: two host threads recording two events per launch slow the
  // profiled pass itself by ~15 % (measured), which would under-report every kernel class
  static const bool prof_lanes = getenv("CM_PROFILE_LANES") != nullptr;
  if (m->profile && !prof_lanes) lanes = 1;
  int Bl[4], off[4];
  hipStream_t sts[4] = {st, m->lane_stream[1], m->lane_stream[2], m->lane_stream[3]};
  for (int ln = 0, o = 0; ln < lanes; ++ln) {
    Bl[ln] = B / lanes + (ln < B % lanes ? 1 : 0);
    off[ln] = o;
    o += Bl[ln];
  }
  // one plan per distinct lane batch (the lanes' batches differ by at most one sample), built here: the lane threads only read them
  FwdPlan odd_plan;
  if (make_plan(m, false, Bl[0], &m->plan) || (Bl[lanes - 1] != Bl[0] && make_plan(m, false, Bl[lanes - 1], &odd_plan))) return 1;
  if (lanes > 1) {
    CM_HIP(hipEventRecord(m->ev_fork, st));
    for (int ln = 1; ln < lanes; ++ln) CM_HIP(hipStreamWaitEvent(sts[ln], m->ev_fork, 0));
  }
  // per-step scalars (host): the same numbers drive the eager launches and the graph's device table
  std::vector<cm::StepRow> rows(order.size());
  for (size_t k = 0; k < order.size(); ++k) {
    const int t = order[k];
    cm::StepRow &r = rows[k];
    r.t = t; r.step = t; r.mass = 0.f;
    if (opts->sampler == CM_SAMPLER_FM_EULER) {
      r.c_x = 1.0f; r.c_eps = (float)(1.0 / (double)opts->fm_steps); r.c_noise = 0.f;  // xt + delta * u, flow_matching.py:219
      r.draw = 0; r.guid = 0.f;
      r.step = (int)k;
    } else if (opts->sampler == CM_SAMPLER_DDIM) {
      const float sab_p = s->tab[CM_TAB_SQRT_ALPHA_BAR][t], s1m_p = s->tab[CM_TAB_SQRT_ONE_MINUS_ALPHA_BAR][t];
      const float sig = opts->ddim_sigma;
      r.c_x = sab_p / sab_t;
      r.c_eps = sqrtf(1.0f - sab_p * sab_p - sig * sig) - sab_p * s1m_t / sab_t;
      r.c_noise = sig;
      r.draw = 1;                                                  // noise on every step (ddpm.py:264)
      r.guid = opts->guidance == CM_GUIDANCE_SPARSITY ? opts->lambda_guidance * sqrtf(beta_t) : 0.f;  // ddpm.py:270
      beta_t = s->tab[CM_TAB_BETA][t]; sab_t = sab_p; s1m_t = s1m_p;
    } else {
      ddpm_coeffs(s, t, &r.c_x, &r.c_eps, &r.c_noise);
      r.draw = t > 0;                                              // ddpm.py:27
      r.guid = opts->guidance == CM_GUIDANCE_SPARSITY ? opts->lambda_guidance * sqrtf(s->tab[CM_TAB_BETA][t]) : 0.f;
      if (mass) {                                                  // (1 - alpha_t) in fp32, alpha_t = 1 - beta_t (ddpm.py:38)
        const float a = 1.0f - s->tab[CM_TAB_BETA][t];
        r.mass = 1.0f - a;
      }
    }
  }
  auto base_args = [&]() {
    cm::StepArgs a{};
    a.C = c.in_channels; a.H = c.rows; a.W = c.cols; a.P = c.past_len; a.F = c.future_len;
    a.seed = opts->seed; a.cs = 8;
    return a;
  };
  // mass_preservation: q of the new x of samples [b0, b0 + Bn), then x -= c q (also into x8 and the history row)
  const size_t per_q = (size_t)3 * c.rows * c.cols * c.future_len;
  auto mass_step = [&](int b0, int Bn, float cmass, float *hist, const cm::StepRow *tab, long long boff, hipStream_t ls) -> int {
    float *x = m->xstate + (size_t)b0 * per;
    float *q = m->mass_q + (size_t)b0 * per_q;
    CM_HIP(cm::launch_mass_grad(x, c.in_channels, q, 3, Bn, c.rows, c.cols, c.future_len, 1.0f, 1.0f, 0.1f, ls));   // ddpm.py:228
    cm::MassApplyArgs ma{};
    ma.x = x; ma.q = q; ma.x8 = m->x8 + (size_t)b0 * m->L() * c.rows * c.cols * 8; ma.hist = hist;
    ma.B = Bn; ma.C = c.in_channels; ma.H = c.rows; ma.W = c.cols; ma.P = c.past_len; ma.F = c.future_len;
    ma.c = cmass; ma.tab = tab; ma.kctr = m->d_kctr; ma.row_stride = (long long)B * per; ma.boff = boff;
    CM_HIP(cm::launch_mass_apply(ma, ls));
    return 0;
  };
  // the UNet's two end convs inside the loop (loop_ends_plan); step 0 of the call always runs the first conv whole: the past has
  // just been assembled, and the weights may have changed since the last call
  const LoopEnds ends = m->dit ? LoopEnds{} : loop_ends_plan(m->ops, m->x8, m->eps_cl, m->loop_ends, m->precision, m->h2_stale, c.past_len,
                                                             c.future_len, c.in_channels, c.out_channels);
  const bool graph = opts->use_graph && !m->profile && lanes == 1 && !stream && order.size() >= 3;
  if (graph) {
    // hipGraph replay: one captured step (the kernels read their per-step scalars from a device table indexed by a
    // device counter), launched once per remaining step.  Step 0 runs eagerly: the launchers set their kernels' function
    // attributes on first use, which may not happen inside a capture (the plan itself is complete since finalize).
    if (m->steptab_cap < rows.size()) {
      if (dev_alloc(m, (void **)&m->d_steptab, rows.size() * sizeof(cm::StepRow))) return 1;
      m->steptab_cap = rows.size();
    }
    if (!m->d_kctr && dev_alloc(m, (void **)&m->d_kctr, sizeof(int))) return 1;
    CM_HIP(hipMemcpyAsync(m->d_steptab, rows.data(), rows.size() * sizeof(cm::StepRow), hipMemcpyHostToDevice, st));
    CM_HIP(hipMemsetAsync(m->d_kctr, 0xFF, sizeof(int), st));   // -1
    CM_HIP(hipStreamSynchronize(st));                            // `rows` is host memory of this call
    auto enqueue_step = [&](bool first) -> int {
      CM_HIP(cm::launch_step_begin(m->tbuf, B, m->d_steptab, m->d_kctr, st));
      cm::StepArgs al = base_args();
      al.B = B; al.x = m->xstate; al.eps_cl = m->eps_cl; al.x8 = m->x8;
      al.sample_id_base = opts->sample_id_base;
      al.tab = m->d_steptab; al.kctr = m->d_kctr; al.row_stride = (long long)B * per; al.boff = 0;
      al.hist = d_history; al.noise = d_noise;
      LoopEnds le = ends;
      le.step = &al;
      if (first) le.tz_first = 0;
      if (denoise(m, m->plan, st, 0, 0, &le)) return 1;
      if (!ends.fuse) CM_HIP(cm::launch_sampler_step(al, st));
      if (mass && mass_step(0, B, 0.f, d_history, m->d_steptab, 0, st)) return 1;
      return 0;
    };
    if (enqueue_step(true)) return 1;
    hipGraph_t g = nullptr;
    hipGraphExec_t ge = nullptr;
    CM_HIP(hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed));
    const int rc_cap = enqueue_step(false);
    hipError_t ec = hipStreamEndCapture(st, &g);
    if (rc_cap || ec != hipSuccess) { if (g) hipGraphDestroy(g); return rc_cap ? 1 : fail("graph capture failed: %s", hipGetErrorString(ec)); }
    ec = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
    if (ec != hipSuccess) { hipGraphDestroy(g); return fail("graph instantiate failed: %s", hipGetErrorString(ec)); }
    for (size_t k = 1; k < order.size() && ec == hipSuccess; ++k) ec = hipGraphLaunch(ge, st);
    if (ec == hipSuccess) ec = hipStreamSynchronize(st);
    hipGraphExecDestroy(ge);
    hipGraphDestroy(g);
    if (ec != hipSuccess) return fail("graph replay failed: %s", hipGetErrorString(ec));
  }
  // steps [k0, k1) of batch lane `ln` on its own stream
  auto lane_steps = [&](int ln, size_t k0, size_t k1) -> int {
    const int b0 = off[ln], Bn = Bl[ln];
    hipStream_t ls = sts[ln];
    for (size_t k = k0; k < k1; ++k) {
      const int t = order[k];
      cm::StepArgs al = base_args();
      const cm::StepRow &r = rows[k];
      al.step = r.step; al.c_x = r.c_x; al.c_eps = r.c_eps; al.c_noise = r.c_noise; al.draw = r.draw; al.guid = r.guid;
      if (k == 0) CM_HIP(cm::launch_fill_t(m->tbuf + b0, Bn, t, ls));
      al.B = Bn;
      if (k + 1 < order.size()) { al.t_next = m->tbuf + b0; al.t_next_v = order[k + 1]; }
      al.x = m->xstate + (size_t)b0 * per;
      al.eps_cl = m->eps_cl + (size_t)b0 * m->L() * c.rows * c.cols * 8;
      al.x8 = m->x8 + (size_t)b0 * m->L() * c.rows * c.cols * 8;
      al.sample_id_base = opts->sample_id_base + b0;
      al.hist = d_history ? d_history + (k + 1) * B * per + (size_t)b0 * per : nullptr;
      al.noise = (d_noise && al.draw) ? d_noise + k * B * per + (size_t)b0 * per : nullptr;
      LoopEnds le = ends;
      le.step = &al;
      if (k == 0) le.tz_first = 0;
      if (denoise(m, Bn == m->plan.ctx.B ? m->plan : odd_plan, ls, b0, ln, &le)) return 1;
      if (!ends.fuse) CM_HIP(cm::launch_sampler_step(al, ls));
      if (mass && mass_step(b0, Bn, r.mass, al.hist, nullptr, 0, ls)) return 1;
    }
    return 0;
  };
  if (!graph && lanes == 1) {
    if (lane_steps(0, 0, order.size())) return 1;
  } else if (!graph) {
    // Step 0 of every lane from the calling thread (the launchers' first-use function attributes are set there, once);
    // the remaining steps of lane ln > 0 are enqueued by a host thread of its own, so that the lanes' launch
    // streams fill independently (one thread alternating between the streams is launch-bandwidth bound).
    for (int ln = 0; ln < lanes; ++ln)
      if (lane_steps(ln, 0, 1)) return 1;
    // (nothing may throw across the C ABI: a worker's exception becomes its lane's error; a lane whose thread cannot be
    //  created is enqueued from the calling thread instead)
    std::vector<int> rcs((size_t)lanes, 0);
    std::vector<std::string> errs((size_t)lanes);
    std::vector<std::thread> workers;
    std::vector<char> started((size_t)lanes, 0);
    try {
      workers.reserve((size_t)lanes);
      for (int ln = 1; ln < lanes; ++ln) {
        try {
          workers.emplace_back([&, ln]() {
            try {
              if (hipSetDevice(m->device) != hipSuccess) { rcs[ln] = 1; errs[ln] = "hipSetDevice failed in a lane thread"; return; }
              rcs[ln] = lane_steps(ln, 1, order.size());
              if (rcs[ln]) errs[ln] = g_err;
            } catch (const std::exception &e) {
              rcs[ln] = 1;
              try { errs[ln] = e.what(); } catch (...) {}
            } catch (...) {
              rcs[ln] = 1;
            }
          });
          started[ln] = 1;
        } catch (...) {
          started[ln] = 0;                        // no thread for this lane: the calling thread enqueues it below
        }
      }
      rcs[0] = lane_steps(0, 1, order.size());
      if (rcs[0]) errs[0] = g_err;
      for (int ln = 1; ln < lanes; ++ln)
        if (!started[ln]) {
          rcs[ln] = lane_steps(ln, 1, order.size());
          if (rcs[ln]) errs[ln] = g_err;
        }
    } catch (const std::exception &e) {
      rcs[0] = 1;
      try { errs[0] = e.what(); } catch (...) {}
    } catch (...) {
      rcs[0] = 1;
    }
    for (auto &w : workers) w.join();
    for (int ln = 0; ln < lanes; ++ln)
      if (rcs[ln]) return fail("lane %d: %s", ln, errs[ln].empty() ? "exception in the lane's enqueue thread" : errs[ln].c_str());
  }
  for (int ln = 1; ln < lanes; ++ln) {
    CM_HIP(hipEventRecord(m->ev_join[ln], sts[ln]));
    CM_HIP(hipStreamWaitEvent(st, m->ev_join[ln], 0));
  }
  CM_HIP(hipMemcpyAsync(d_out, m->xstate, B * per * sizeof(float), hipMemcpyDeviceToDevice, st));
  if (opts->check_finite) {
    // sampler-output health check: a NaN / Inf from a bad checkpoint must not come back as rc 0
    if (!m->d_nonfinite && dev_alloc(m, (void **)&m->d_nonfinite, sizeof(int))) return 1;
    CM_HIP(cm::launch_count_nonfinite(m->xstate, (long long)(B * per), m->d_nonfinite, st));
    int bad = 0;
    CM_HIP(hipMemcpyAsync(&bad, m->d_nonfinite, sizeof(int), hipMemcpyDeviceToHost, st));
    CM_HIP(hipStreamSynchronize(st));
    if (prof_collect(m, st)) return 1;
    if (bad) return fail("sampling produced %d non-finite values out of %lld (check_finite)", bad, (long long)(B * per));
    return 0;
  }
  return prof_collect(m, st);
}

int cm_sample_loop_host(cm_model *m, const cm_schedule *s, const float *h_past, const float *h_xT, const float *h_noise,
                        const cm_sample_opts *opts, float *h_out, float *h_history, int32_t B) {
  if (check_ready(m, B)) return 1;
  if (!s || !h_past || !opts || !h_out) return fail("null argument");
  DevGuard g(m->device);
  const cm_unet_config &c = m->cfg;
  const size_t per = (size_t)m->per_sample();
  const size_t per_past = (size_t)c.in_channels * c.rows * c.cols * c.past_len;
  const size_t nsteps = visit_order(s, opts).size();
  CM_HIP(hipMemcpy(m->stage_past, h_past, B * per_past * sizeof(float), hipMemcpyHostToDevice));
  if (h_xT) CM_HIP(hipMemcpy(m->stage_fut, h_xT, B * per * sizeof(float), hipMemcpyHostToDevice));
  float *dn = nullptr, *dh = nullptr;
  if (h_noise) {
    CM_HIP(hipMalloc((void **)&dn, nsteps * B * per * sizeof(float)));
    hipError_t e = hipMemcpy(dn, h_noise, nsteps * B * per * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) { hipFree(dn); return fail("noise upload failed: %s", hipGetErrorString(e)); }
  }
  if (h_history) {
    hipError_t e = hipMalloc((void **)&dh, (nsteps + 1) * B * per * sizeof(float));
    if (e != hipSuccess) { if (dn) hipFree(dn); return fail("history alloc failed: %s", hipGetErrorString(e)); }
  }
  int rc = cm_sample_loop(m, s, m->stage_past, h_xT ? m->stage_fut : nullptr, dn, opts, m->stage_out, dh, B, nullptr);
  if (!rc) {
    hipError_t e = hipStreamSynchronize(m->stream);
    if (e != hipSuccess) rc = fail("sampling loop failed: %s", hipGetErrorString(e));
  }
  if (!rc) {
    hipError_t e = hipMemcpy(h_out, m->stage_out, B * per * sizeof(float), hipMemcpyDeviceToHost);
    if (e == hipSuccess && h_history) e = hipMemcpy(h_history, dh, (nsteps + 1) * B * per * sizeof(float), hipMemcpyDeviceToHost);
    if (e != hipSuccess) rc = fail("result download failed: %s", hipGetErrorString(e));
  }
  if (dn) hipFree(dn);
  if (dh) hipFree(dh);
  return rc;
}

int cm_profile_enable(cm_model *m, int32_t on) {
  CM_NOT_DIT(m, "cm_profile_enable");
  if (!m) return fail("null model handle");
  m->profile = on != 0;
  return 0;
}

int cm_profile_read(cm_model *m, float ms[8], int64_t launches[8]) {
  CM_NOT_DIT(m, "cm_profile_read");
  if (!m || !ms || !launches) return fail("null argument");
  for (int i = 0; i < 8; ++i) { ms[i] = m->prof_ms[i]; launches[i] = m->prof_n[i]; }
  return 0;
}

int cm_profile_read_union(cm_model *m, float ms[8]) {
  CM_NOT_DIT(m, "cm_profile_read_union");
  if (!m || !ms) return fail("null argument");
  for (int i = 0; i < 8; ++i) ms[i] = m->prof_union_ms[i];
  return 0;
}

int cm_model_cost(const cm_model *m, int32_t B, double *flops, double *bytes) {
  if (!m || !m->finalized) return fail("model not finalized");
  if (m->dit) return dit_cost(m, B, flops, bytes);
  double f = 0, by = 0;
  for (const Op &op : m->ops) {
    if (op.kind == OP_CONV) {
      f += op.flops_per_sample * B;
      const cm::ConvArgs &a = op.ca;
      const double vin = (double)a.Zs * a.Ys * a.Xs, vout = (double)a.Zo * a.Yo * a.Xo;
      by += 4.0 * B * (vin * (a.C0 + a.C1) + vout * a.Co);
    } else if (op.kind == OP_ATTN) {
      f += 4.0 * op.S * (double)op.S * op.E * B;
    }
  }
  double wbytes = 0;
  for (const Param &p : m->params) wbytes += 4.0 * p.numel();
  if (flops) *flops = f;
  if (bytes) *bytes = by + wbytes;
  return 0;
}

int cm_profile_report(cm_model *m, char *buf, int64_t capacity) {
  CM_NOT_DIT(m, "cm_profile_report");
  if (!m || !buf || capacity < 1) return fail("null argument");
  std::string out;
  char line[512];
  for (const Op &op : m->ops) {
    if (op.prof_n == 0) continue;
    const double us = op.prof_ms * 1e3 / op.prof_n;
    if (op.kind == OP_CONV) {
      const cm::ConvArgs &a = op.ca;
      const double tf = op.flops_per_sample * m->prof_B / (us * 1e-6) / 1e12;
      snprintf(line, sizeof(line), "%-52s %9.1f us %7.2f TF %8.1f MF/sample B%d ks%d  %s%d NB%d box %dx%dx%dx%d grid %dx%d CK%d lds %zu\n", op.label.c_str(), us, tf,
               op.flops_per_sample / 1e6, m->prof_B, op.ks,
               "MB", op.MB, op.NB, a.bs, a.bz, a.by, a.bx, a.nts * a.ntz * a.nty * a.ntx,
               (a.Co + 32 * op.NB - 1) / (32 * op.NB), a.CK, cm::conv_lds_bytes(a, op.MB, op.NB));
    } else {
      snprintf(line, sizeof(line), "%-52s %9.1f us\n", op.label.c_str(), us);
    }
    out += line;
  }
  snprintf(buf, (size_t)capacity, "%s", out.c_str());
  return 0;
}

// ---- sampling metrics: the reductions of utils/metrics/metricsGenerator.py on the device ------
int cm_frame_metrics(int32_t device, const float *d_pred, const float *d_gt, int32_t N, int32_t Cc, int32_t H, int32_t W,
                     int32_t F, double *h_out, float *h_minmax) {
  if (!d_pred || !d_gt || !h_out || !h_minmax) return fail("null argument");
  if (N < 1 || Cc < 1 || H < 1 || W < 1 || F < 1) return fail("bad shape");
  DevGuard g(device);
  const size_t cells = (size_t)N * Cc * F;
  double *d_out = nullptr;
  float *d_mm = nullptr;
  CM_HIP(hipMalloc((void **)&d_out, cells * 8 * sizeof(double)));
  hipError_t e = hipMalloc((void **)&d_mm, cells * 2 * sizeof(float));
  if (e == hipSuccess) e = cm::launch_frame_metrics(d_pred, d_gt, N, Cc, H, W, F, d_out, d_mm, nullptr);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(h_out, d_out, cells * 8 * sizeof(double), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(h_minmax, d_mm, cells * 2 * sizeof(float), hipMemcpyDeviceToHost);
  hipFree(d_out);
  if (d_mm) hipFree(d_mm);
  if (e != hipSuccess) return fail("frame metrics failed: %s", hipGetErrorString(e));
  return 0;
}

int cm_mass_preservation_grad(int32_t device, const float *d_x, int32_t B, int32_t Cc, int32_t H, int32_t W, int32_t L,
                              float delta_t, float delta_l, float eps, float *d_grad, void *stream) {
  if (!d_x || !d_grad) return fail("null argument");
  if (B < 1 || H < 1 || W < 1 || L < 1) return fail("bad shape [%d,%d,%d,%d,%d]", B, Cc, H, W, L);
  if (Cc < 3) return fail("mass_preservation gradient needs >= 3 channels (r, u, v: guidance.py:25-31), got %d", Cc);
  if (delta_t == 0.f || delta_l == 0.f) return fail("delta_t and delta_l must be non-zero");
  if (d_x == d_grad) return fail("d_grad must not alias d_x (the gradient is written out of place)");
  DevGuard g(device);
  CM_HIP(cm::launch_mass_grad(d_x, Cc, d_grad, Cc, B, H, W, L, delta_t, delta_l, eps, (hipStream_t)stream));
  return 0;
}

// ---- tile tuner hooks (tools/tune_tiles.py; not used by the product path) --------------------
int cm_debug_conv_flags(int32_t flags) {
  cm::conv_dbg_override = flags;   // < 0: back to the CM_CONV_DBG environment value
  return 0;
}

int cm_debug_conv_count(const cm_model *m, int32_t *count) {
  CM_NOT_DIT(m, "cm_debug_conv_count");
  if (!m || !m->finalized || !count) return fail("model not finalized");
  *count = (int32_t)m->ops.size();
  return 0;
}

// One line per op: "conv <label> ntaps stride par Ci Co Zo Yo Xo NB MB bz by bx ks flags out_C C0 C1 wino kernel form" or "other <label>";
// kernel (a name of kConvKernelName) and form (a ConvForm number) are the op's inference route (conv_route).  A fused attention block:
// "other <label> attn_sample_kernel" or "... attn_head_kernel", what the handle's inference plan launches for it.
namespace {
int conv_info_line(const cm_model *m, int32_t index, char *buf, int64_t capacity, bool ext) {
  if (!m || !m->finalized || !buf || index < 0 || index >= (int)m->ops.size()) return fail("bad argument");
  const Op &op = m->ops[index];
  if (op.kind == OP_ATTNBLK) {   // ... "other <label> <kernel>": what the handle's inference plan launches for the block
    const FwdPlan pl = plan_forward(m->ops, FwdCtx{m->precision, false, m->h2_stale, m->plan.ctx.B});
    snprintf(buf, (size_t)capacity, "other %s %s", op.label.c_str(), pl.ops[index].attn_sample ? "attn_sample_kernel" : "attn_head_kernel");
    return 0;
  }
  if (op.kind == OP_GNFIN && m->plan.err.empty() && m->plan.ops.size() == m->ops.size() && m->plan.ops[index].fin != FIN_NONE) {
    // ... "other <label> fin <who> <ns0> <ns1>": who merged this GroupNorm's slots in the last forward, and how many slots per source
    static const char *const who[] = {"none", "qr", "combine", "wino", "alone"};
    const OpPlan &p = m->plan.ops[index];
    snprintf(buf, (size_t)capacity, "other %s fin %s %d %d", op.label.c_str(), who[p.fin], p.ns0, p.ns1);
    return 0;
  }
  if (op.kind != OP_CONV) { snprintf(buf, (size_t)capacity, "other %s", op.label.c_str()); return 0; }
  const cm::ConvArgs &a = op.ca;
  const ConvRoute r = conv_route(op, m->precision, false, m->h2_stale);
  // after them, for the two end convs of the UNet: what a sampling-loop step leaves out ("loop_ztiles <first tile of later steps>/<ntz>",
  // 0 = every step launches all tiles; "loop_planes <first>:<end> fuse <variant>")
  const LoopEnds le = loop_ends_plan(m->ops, m->x8, m->eps_cl, m->loop_ends, m->precision, m->h2_stale, m->cfg.past_len, m->cfg.future_len,
                                     m->cfg.in_channels, m->cfg.out_channels);
  char tail[192] = "";
  if (r.kernel == CONV_FIRST && a.src0 == m->x8) snprintf(tail, sizeof tail, " loop_ztiles %d/%d", le.tz_first, a.ntz);
  if (r.kernel == CONV_FIN && a.out == m->eps_cl && le.zo_end) snprintf(tail, sizeof tail, " loop_planes %d:%d fuse %d", le.zo_first, le.zo_end, le.fuse);
  // ... then, through cm_debug_conv_info_ext only (cm_debug_conv_info's line stays what its readers compare whole tails of), for
  // every conv: "h16 <h16_mask of the product launch> res <channel stride of the residual tensor, 0 = none> skip <C of the
  // fused skip conv's two sources, 0 0 = none>", and for the direct f16 kernel / the stage-once upsample conv the tile of its own that the
  // statistics slots follow: "f16d <bz> <by> <bx> <mbw>" / "upst <tz> <ty> <tx> <mbw>"; for an absorbed skip conv "alone ..." (below)
  if (ext) {
    const size_t n = strlen(tail);
    const bool fused = op.d_s2w != nullptr;
    snprintf(tail + n, sizeof tail - n, " h16 %d res %d skip %d %d", h16_mask(op, false), (!fused && op.resid_act) ? op.resid_act->C : 0,
             fused ? op.skip0->C : 0, (fused && op.skip1) ? op.skip1->C : 0);
    const size_t n2 = strlen(tail);
    if (r.kernel == CONV_F16D) snprintf(tail + n2, sizeof tail - n2, " f16d %d %d %d %d", op.f16d_bz, op.f16d_by, op.f16d_bx, op.f16d_mbw);
    if (r.kernel == CONV_UPS) snprintf(tail + n2, sizeof tail - n2, " upst %d %d %d %d", op.ups_tz, op.ups_ty, op.ups_tx, op.ups_mbw);
    if (op.skip_if_fused) {   // kernel "none": "alone <kernel> <form>", the route cm_debug_conv_io launches it on (as its own op, raw)
      Op alone = op; alone.skip_if_fused = false; alone.dbg_raw = true;
      const ConvRoute ra = conv_route(alone, m->precision, false, m->h2_stale);
      snprintf(tail + n2, sizeof tail - n2, " alone %s %d", kConvKernelName[ra.kernel], (int)ra.form);
    }
  }
  snprintf(buf, (size_t)capacity, "conv %s %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %s %d%s", op.label.c_str(), a.ntaps, a.stride, a.par,
           a.C0 + a.C1, a.Co, a.Zo, a.Yo, a.Xo, op.NB, op.MB, a.bz, a.by, a.bx, op.ks,
           (op.small_n ? 1 : 0) | (op.first_k ? 2 : 0) | (op.stat_act ? 4 : 0) | (op.skip_if_fused ? 8 : 0) | (a.CK == 32 ? 16 : 0),
           op.out_act ? op.out_act->C : a.Co,        // (channel stride of the output tensor, cm_debug_conv_io's h_out)
           a.C0, a.C1, op.wino ? 1 : 0,              // (channels of the two sources; does the Winograd launcher take the op)
           kConvKernelName[r.kernel], (int)r.form, tail);
  return 0;
}
}  // namespace

int cm_debug_conv_info(const cm_model *m, int32_t index, char *buf, int64_t capacity) {
  CM_NOT_DIT(m, "cm_debug_conv_info");
  return conv_info_line(m, index, buf, capacity, false);
}

// Test hook, exported like cm_debug_loop_ends (tests/test_gpu_f16_layers.py): cm_debug_conv_info's line with, on a "conv" line, the
// trailing tokens described in conv_info_line appended (f16-tensor mask, residual / fused skip channels, the direct f16 / stage-once
// upsample kernel's own tile, the stand-alone route of an absorbed skip conv).
extern "C" int cm_debug_conv_info_ext(const cm_model *m, int32_t index, char *buf, int64_t capacity) {
  CM_NOT_DIT(m, "cm_debug_conv_info_ext");
  return conv_info_line(m, index, buf, capacity, true);
}

// Test hook, exported but outside the public header (the binding table is fixed): which of the loop's end-conv savings the handle
// takes (cm_model::loop_ends; 0 restores whole convs and the separate sampler launch, 7 is the default).
extern "C" int cm_debug_loop_ends(cm_model *m, int32_t mask) {
  CM_NOT_DIT(m, "cm_debug_loop_ends");
  if (!m || mask < 0 || mask > 15) return fail("bad argument");
  m->loop_ends = mask;
  return 0;
}

// Test hook, exported like cm_debug_loop_ends (tests/test_gpu_attn_sample.py): the fused attention block at op `index` ALONE on the
// caller's input h_x (host, channels-last [B][S][E]).  mode 0: the (head, sample) launch and the head sum; mode 1: the whole-sample
// launch -- an error, never the other path, where this handle's inference plan at batch B does not take it.  The hook's second pass
// carries no finalisation.  h_out: [B][S][E]; h_part / h_cnt (may be null): the slot statistics written, [B][ceil(S / 32)][E][2]
// (mean, M2) and [B][ceil(S / 32)].
extern "C" int cm_debug_attn_block(cm_model *m, int32_t index, int32_t mode, const float *h_x, float *h_out, float *h_part, float *h_cnt,
                                   int32_t B) {
  CM_NOT_DIT(m, "cm_debug_attn_block");
  if (check_ready(m, B)) return 1;
  if (!h_x || !h_out || index < 0 || index >= (int)m->ops.size() || mode < 0 || mode > 1) return fail("bad argument");
  const Op &op = m->ops[index];
  if (op.kind != OP_ATTNBLK) return fail("op %d is not a fused attention block", index);
  DevGuard g(m->device);
  if (m->h2_stale && refresh_h2(m)) return 1;
  FwdPlan plan;
  if (make_plan(m, false, B, &plan)) return 1;
  OpPlan &p = plan.ops[index];
  if (mode == 1 && !p.attn_sample) return fail("op %d: the plan does not take the whole-sample attention kernel", index);
  p.attn_sample = mode == 1; p.carries = -1;
  hipStream_t st = m->stream;
  const size_t n = (size_t)B * op.S * op.E;
  CM_HIP(hipMemcpy(op.ab_x->d, h_x, n * sizeof(float), hipMemcpyHostToDevice));
  const int rc = run_attn_block(m, op, plan, p, st, 0, 0);
  const hipError_t e = hipStreamSynchronize(st);
  if (rc) return 1;
  if (e != hipSuccess) return fail("debug attention launch failed: %s", hipGetErrorString(e));
  CM_HIP(hipMemcpy(h_out, op.ab_out->d, n * sizeof(float), hipMemcpyDeviceToHost));
  if (h_part) CM_HIP(hipMemcpy(h_part, op.ab_out->part, (size_t)B * p.ns_out * op.E * 2 * sizeof(float), hipMemcpyDeviceToHost));
  if (h_cnt) CM_HIP(hipMemcpy(h_cnt, op.ab_out->cnt, (size_t)B * p.ns_out * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}

// Test hook (tests/test_gpu_attn_sample.py, tests/test_attn_sample_cpu.py): the host-side pack of the whole-sample attention kernel's
// weight fragments.  w: [N][K] (N % 16 == 0, K % 32 == 0); halves: N * K * 2 f16 bit patterns in the kernel's order
// ([N / 16][K / 32][hi, mid][64 lanes][8]); *scale: the power of two the weights were multiplied by (0: none).  No device is touched.
extern "C" int cm_debug_attn_pack(const float *w, int32_t N, int32_t K, uint16_t *halves, float *scale) {
  if (!w || !halves || !scale || N < 16 || K < 32 || N % 16 || K % 32) return fail("bad argument");
  *scale = h2_wscale(w, (size_t)N * K);
  const std::vector<float> f = pack_attn_h2(w, N, K, *scale);
  std::memcpy(halves, f.data(), f.size() * sizeof(float));
  return 0;
}

// ... and its shape predicate (1: the whole-sample kernel admits S tokens of E channels in `heads` heads and `groups` groups)
extern "C" int cm_debug_attn_sample_ok(int32_t S, int32_t E, int32_t heads, int32_t groups) { return cm::attn_sample_ok(S, E, heads, groups) ? 1 : 0; }

namespace {
// Host data <-> an activation of the handle, honouring Act::h16 (plan_h16).  An h16 tensor keeps the allocation new_act gave it --
// max_batch * V * C FLOATS, made before plan_h16 runs and never resized -- and uses its first half: the same [B][Z][Y][X][C] order
// in _Float16 elements (run_conv's `adv` halves the float offset).  Upload rounds to nearest even, overflow to infinity
// (f32_to_f16_bits = the kernels' (_Float16) casts); download fetches the halves as stored and widens them, as cm_debug_activation does.
int dbg_upload(const Act *t, const float *h, size_t n) {
  if (!t->h16) { CM_HIP(hipMemcpy(t->d, h, n * sizeof(float), hipMemcpyHostToDevice)); return 0; }
  std::vector<uint16_t> raw(n);
  for (size_t i = 0; i < n; ++i) raw[i] = f32_to_f16_bits(h[i]);
  CM_HIP(hipMemcpy(t->d, raw.data(), n * sizeof(uint16_t), hipMemcpyHostToDevice));
  return 0;
}
int dbg_download(const Act *t, float *h, size_t n) {
  if (!t->h16) { CM_HIP(hipMemcpy(h, t->d, n * sizeof(float), hipMemcpyDeviceToHost)); return 0; }
  std::vector<uint16_t> raw(n);
  CM_HIP(hipMemcpy(raw.data(), t->d, n * sizeof(uint16_t), hipMemcpyDeviceToHost));
  for (size_t i = 0; i < n; ++i) h[i] = f16_bits_to_f32(raw[i]);
  return 0;
}

// cm_debug_conv_io / cm_debug_conv_tail.  `tail`: the raw launch keeps the op's residual or fused skip conv, on the caller's data h_t0 / h_t1.
int debug_conv_launch(cm_model *m, int32_t index, int32_t mode, bool tail, const float *h_in0, const float *h_in1, const float *h_t0,
                      const float *h_t1, float *h_out, int32_t B) {
  if (check_ready(m, B)) return 1;
  if (!h_in0 || !h_out || index < 0 || index >= (int)m->ops.size()) return fail("bad argument");
  const Op &op = m->ops[index];
  if (op.kind != OP_CONV || !op.in0 || !op.out_act) return fail("op %d is not a convolution", index);
  if ((op.in1 != nullptr) != (h_in1 != nullptr)) return fail("op %d has %d source tensors", index, op.in1 ? 2 : 1);
  const bool fused = op.d_s2w != nullptr;
  const Act *t0 = !tail ? nullptr : fused ? op.skip0 : op.resid_act, *t1 = (tail && fused) ? op.skip1 : nullptr;
  if (tail) {
    if (!t0) return fail("op %d has neither a residual nor a fused skip conv", index);
    if ((t0 != nullptr) != (h_t0 != nullptr) || (t1 != nullptr) != (h_t1 != nullptr))
      return fail("op %d takes %d tensor(s) behind its %s", index, t1 ? 2 : 1, fused ? "fused skip conv" : "residual");
    for (const Act *t : {t0, t1})
      if (t && (t == op.in0 || t == op.in1 || t == op.out_act)) return fail("op %d: a residual / skip tensor is also a source or the output", index);
  }
  DevGuard g(m->device);
  hipStream_t st = m->stream;
  const size_t Vs = (size_t)op.in0->V(), Vo = (size_t)op.out_act->V();
  if (dbg_upload(op.in0, h_in0, (size_t)B * Vs * op.in0->C)) return 1;
  if (op.in1 && dbg_upload(op.in1, h_in1, (size_t)B * Vs * op.in1->C)) return 1;
  if (t0 && dbg_upload(t0, h_t0, (size_t)B * Vo * t0->C)) return 1;
  if (t1 && dbg_upload(t1, h_t1, (size_t)B * Vo * t1->C)) return 1;
  if (mode < 0 || mode > 3) return fail("mode %d", mode);
  // Modes 1 and 2 name operand forms of the fp32 plans.  The reduced-precision plan has one form per conv -- conv_route takes the f16
  // fragments whatever the op's debug flags say -- so on such a handle they ARE mode 0, for every op (its quarter-resolution convs
  // included: nothing is withheld, no source statistics are recomputed).
  if (m->precision == CM_PRECISION_F16 && (mode == 1 || mode == 2)) mode = 0;
  Op tmp = op;
  if (mode != 3) {
    tmp.ca.gn = nullptr; tmp.ca.silu = 0; tmp.ca.temb = nullptr; tmp.temb_off = -1; tmp.dbg_raw = true; tmp.pm_off = -1;
    if (!tail) { tmp.ca.resid = nullptr; tmp.resid_act = nullptr; tmp.d_s2w = nullptr; tmp.d_wqr_skip = nullptr; }
    if (!tmp.qr) tmp.gn_op = -1;
  }
  tmp.skip_if_fused = false;
  tmp.dbg_h2 = mode == 2;
  if (mode == 1) { tmp.d_wwino_b6 = nullptr; tmp.d_wqr_b6 = nullptr; tmp.d_wups_b6 = nullptr; }
  int src_slots = 0;
  if (mode == 2 && op.ups && op.in0->part) {
    // the upsample conv's h2 form scales each sample by its source's slot statistics: the caller's data, in nslice slots, this launch only
    const Act *t = op.in0;
    src_slots = t->nslice;
    CM_HIP(cm::launch_chan_stats(t->d, B, t->V(), t->C, src_slots, t->part, t->cnt, st));
  }
  FwdPlan plan;
  const int rc = plan_debug_conv(m, tmp, index, B, src_slots, st, &plan) || run_conv(m, tmp, plan, plan.ops[index], st, 0, 0);
  const hipError_t e = hipStreamSynchronize(st);
  if (rc) return 1;
  if (e != hipSuccess) return fail("debug conv launch failed: %s", hipGetErrorString(e));
  return dbg_download(op.out_act, h_out, (size_t)B * Vo * op.out_act->C);
}
}  // namespace

// Test hook (tests/test_gpu_six_term_hostile.py): conv op `index` ALONE on the caller's data -- no GroupNorm / SiLU on load, no
// time-embedding row, no residual, no fused skip conv; the bias stays.  h_in0 / h_in1: host, channels-last
// [B][Zs][Ys][Xs][C0 / C1] (h_in1 null when the op has one source); h_out: host [B][Zo][Yo][Xo][channel stride of the output
// tensor].  mode 0: the six-term bf16 form where the plan has one (raw operands are unbounded: never the h2 form); mode 1: the
// same layer on fp32 matrix instructions (the split fragments withheld); mode 2: the h2 form where the plan has one (the caller
// keeps its operands inside the bound the plan guarantees, tests/test_gpu_h2.py); mode 3: the op exactly as the sampling forward
// launches it -- GroupNorm + SiLU on load, time-embedding row, residual, fused skip conv, h2 where the plan has it -- on the caller's
// sources; the GroupNorm rows / slot partials, the time rows, the residual and the skip conv's source are what the last forward
// left (tests/test_gpu_wino_forms.py compares two kernels for the SAME launch with it; cm_debug_conv_stats reads the slots it wrote).
// A handle on the reduced-precision plan: tensors plan_h16 stores as _Float16 are converted on the way in (round to nearest even) and
// out, and modes 1 and 2 EQUAL mode 0 there (one operand form per conv; debug_conv_launch).  An fp32 handle's launches are unchanged.
int cm_debug_conv_io(cm_model *m, int32_t index, int32_t mode, const float *h_in0, const float *h_in1, float *h_out, int32_t B) {
  CM_NOT_DIT(m, "cm_debug_conv_io");
  return debug_conv_launch(m, index, mode, false, h_in0, h_in1, nullptr, nullptr, h_out, B);
}

// Test hook, exported like cm_debug_attn_block (tests/test_gpu_f16_layers.py): the raw single launch of cm_debug_conv_io's mode 0 --
// no GroupNorm / SiLU on load, no time-embedding row -- that KEEPS the tail of the op's inference launch, on the caller's data: the
// residual (h_t0: [B][Zo][Yo][Xo][C of the residual tensor], h_t1 null), or, where the block's 1x1x1 skip conv is fused in, that conv
// over its one or two raw sources (h_t0 / h_t1: [B][Zo][Yo][Xo][C of skip0 / skip1]; the bias is then conv bias + skip bias).  Which of
// the two, and the channel counts: the "res" / "skip" tokens of cm_debug_conv_info.  An op with neither is an error.
extern "C" int cm_debug_conv_tail(cm_model *m, int32_t index, const float *h_in0, const float *h_in1, const float *h_t0, const float *h_t1,
                                  float *h_out, int32_t B) {
  CM_NOT_DIT(m, "cm_debug_conv_tail");
  return debug_conv_launch(m, index, 0, true, h_in0, h_in1, h_t0, h_t1, h_out, B);
}

// Test hook (tests/test_gpu_f16_layers.py): one attention core launch ALONE on host data, no handle -- f16 != 0: launch_attn_core_f16
// (the reduced-precision plan's kernel, 32 channels per head), else launch_attn_core -- on the current device's default stream.
// h_qkv: [B][S][3 E] (q | k | v per token, heads contiguous inside each); h_out: [B][S][E].
extern "C" int cm_debug_attn_core(const float *h_qkv, float *h_out, int32_t B, int32_t S, int32_t E, int32_t heads, int32_t f16) {
  if (!h_qkv || !h_out || B < 1 || S < 1 || E < 1 || heads < 1) return fail("bad argument");
  const size_t nq = (size_t)B * S * 3 * E, no = (size_t)B * S * E;
  float *d_qkv = nullptr, *d_out = nullptr;
  hipError_t e = hipMalloc((void **)&d_qkv, nq * sizeof(float));
  if (e == hipSuccess) e = hipMalloc((void **)&d_out, no * sizeof(float));
  if (e == hipSuccess) e = hipMemcpy(d_qkv, h_qkv, nq * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(d_out, 0xff, no * sizeof(float));      // (NaN wherever the kernel writes nothing)
  if (e == hipSuccess) e = (f16 ? cm::launch_attn_core_f16 : cm::launch_attn_core)(d_qkv, d_out, B, S, E, heads, nullptr);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(h_out, d_out, no * sizeof(float), hipMemcpyDeviceToHost);
  hipFree(d_qkv); hipFree(d_out);
  if (e != hipSuccess) return fail("debug attention core launch failed: %s", hipGetErrorString(e));
  return 0;
}

// Launches of the table-driven Winograd kernel per launch form (cm::conv_wino_form; index 0 = the generic kernel) since the last reset.
int cm_debug_wino_form_counts(int64_t counts[16], int32_t reset) {
  if (!counts) return fail("bad argument");
  long long c[16];
  cm::conv_wino_form_counts(c, reset != 0);
  for (int i = 0; i < 16; ++i) counts[i] = (int64_t)c[i];
  return 0;
}

// ... and how many of them took the halo-ahead order (cm::WINO_FORM_AHEAD; none under CM_DIAG=1 CM_NO_WINO_AHEAD=1).
int cm_debug_wino_ahead_count(int64_t *launches, int32_t reset) {
  if (!launches) return fail("bad argument");
  *launches = (int64_t)cm::conv_wino_ahead_count(reset != 0);
  return 0;
}

// ... and how many staged the next chunk under the matrix phase (cm::WINO_FORM_UNDER; none under CM_DIAG=1 CM_NO_WINO_UNDER=1).
int cm_debug_wino_under_count(int64_t *launches, int32_t reset) {
  if (!launches) return fail("bad argument");
  *launches = (int64_t)cm::conv_wino_under_count(reset != 0);
  return 0;
}

// The statistics slots conv op `index` writes for its output tensor in the last forward's plan: h_part [B][nslots][C][2] (mean, M2), h_cnt
// [B][nslots] rows behind each slot.  h_part / h_cnt may be null: only *nslots / *C are returned (size the buffers, call again).
int cm_debug_conv_stats(cm_model *m, int32_t index, int32_t B, float *h_part, float *h_cnt, int32_t *nslots, int32_t *C) {
  CM_NOT_DIT(m, "cm_debug_conv_stats");
  if (check_ready(m, B)) return 1;
  if (!nslots || !C || index < 0 || index >= (int)m->ops.size()) return fail("bad argument");
  const Op &op = m->ops[index];
  if (op.kind != OP_CONV || !op.stat_act || !op.stat_act->part) return fail("op %d writes no statistics", index);
  const Act *t = op.stat_act;
  const int ns = (size_t)index < m->plan.ops.size() ? m->plan.ops[index].ns_out : 0;   // of the last forward's plan
  *nslots = ns; *C = t->C;
  DevGuard g(m->device);
  CM_HIP(hipStreamSynchronize(m->stream));
  if (h_part) CM_HIP(hipMemcpy(h_part, t->part, (size_t)B * ns * t->C * 2 * sizeof(float), hipMemcpyDeviceToHost));
  if (h_cnt) CM_HIP(hipMemcpy(h_cnt, t->cnt, (size_t)B * ns * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}

// Average duration (us) of `iters` back-to-back launches of conv op `index` at batch B with the tile
// geometry (MB; bz,by,bx) -- 0 keeps the op's own.  The activations are whatever the last forward left.
int cm_debug_time_conv(cm_model *m, int32_t index, int32_t MB, int32_t bz, int32_t by, int32_t bx, int32_t B,
                       int32_t iters, float *us) {
  CM_NOT_DIT(m, "cm_debug_time_conv");
  if (check_ready(m, B)) return 1;
  if (!us || index < 0 || index >= (int)m->ops.size() || iters < 1) return fail("bad argument");
  const Op &own = m->ops[index];
  if (own.kind != OP_CONV || ((own.first_k || own.wino) && MB > 0)) return fail("op %d is not a tunable convolution", index);
  DevGuard g(m->device);
  hipStream_t st = m->stream;
  Op op = own; op.skip_if_fused = false;   // the timed copy: the list keeps the op's own geometry (the device tables are shared, see below)
  int rc = 0;
  if (MB > 0) {
    cm::ConvArgs &a = op.ca;
    const int osd = a.par ? 2 : 1;
    if (bz < 1 || by < 1 || bx < 1 || (bz * by * bx + 31) / 32 != MB || !cm::conv_variant_exists(MB, op.NB)) rc = fail("invalid geometry");
    if (!rc) {
      a.bs = 1; a.bz = bz; a.by = by; a.bx = bx;
      op.MB = MB;
      a.ntz = (a.Zo / osd + bz - 1) / bz; a.nty = (a.Yo / osd + by - 1) / by; a.ntx = (a.Xo / osd + bx - 1) / bx;
      if (cm::conv_lds_bytes(a, MB, op.NB) > 80 * 1024) rc = fail("tile needs too much LDS");  // two workgroups per CU
      if (!rc && op.small_n && (MB & (MB - 1))) rc = fail("small-N kernel needs a power-of-two MB");
      if (!rc && cm::conv_halo_voxels(a) > 16384) rc = fail("halo box too large");
    }
    if (!rc) {
      std::vector<int> hv((size_t)cm::conv_halo_voxels(a)), mt((size_t)32 * MB);
      cm::conv_build_tables(a, MB, hv.data(), mt.data());
      hipError_t e = hipMemcpy(op.d_hvtab, hv.data(), hv.size() * sizeof(int), hipMemcpyHostToDevice);
      if (e == hipSuccess) e = hipMemcpy(op.d_mtab, mt.data(), mt.size() * sizeof(int), hipMemcpyHostToDevice);
      if (e != hipSuccess) rc = fail("table upload failed");
    }
  }
  FwdPlan plan;
  if (!rc) rc = plan_debug_conv(m, op, index, B, 0, st, &plan);
  if (!rc) {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipEventCreate(&e0); hipEventCreate(&e1);
    for (int i = 0; i < 2 && !rc; ++i) rc = run_conv(m, op, plan, plan.ops[index], st, 0, 0);
    hipEventRecord(e0, st);
    for (int i = 0; i < iters && !rc; ++i) rc = run_conv(m, op, plan, plan.ops[index], st, 0, 0);
    hipEventRecord(e1, st);
    hipError_t e = hipStreamSynchronize(st);
    if (!rc && e != hipSuccess) rc = fail("timed launch failed: %s", hipGetErrorString(e));
    float ms = 0.f;
    if (!rc) { hipEventElapsedTime(&ms, e0, e1); *us = ms * 1e3f / (float)iters; }
    hipEventDestroy(e0); hipEventDestroy(e1);
  }
  // the device tables back to the op's own geometry
  if (MB > 0) {
    std::vector<int> hv((size_t)cm::conv_halo_voxels(own.ca)), mt((size_t)32 * own.MB);
    cm::conv_build_tables(own.ca, own.MB, hv.data(), mt.data());
    CM_HIP(hipMemcpy(own.d_hvtab, hv.data(), hv.size() * sizeof(int), hipMemcpyHostToDevice));
    CM_HIP(hipMemcpy(own.d_mtab, mt.data(), mt.size() * sizeof(int), hipMemcpyHostToDevice));
  }
  return rc;
}

// Matrix-core FLOPs the plan actually EXECUTES per kernel class (<= the algorithmic count: the parity form of the
// upsample convs runs 8 of 27 taps, the Winograd layers 16 multiplies per 2x2 outputs and z tap instead of 36,
// computed on whole 32-row blocks and shifted tiles; padding rows of partly filled tiles are counted as executed).
// `b16`, when given, receives the part of those FLOPs that is issued as 16-bit-operand matrix instructions, in ISSUED FLOPs:
// a six-term layer (fp32 products from exact three-way bf16 splits) issues six v_mfma_f32_32x32x16_bf16 products per
// fp32-equivalent product, an f16-plan layer one; `flops` then keeps the part issued as fp32 matrix instructions.
// `train_f16`, when given, switches to the TRAINING forward in the handle's current mode (cm_train_set_autocast) and receives the
// executed FLOPs of the convs on f16 operands; `flops` then holds all executed FLOPs.
static int exec_flops_split(const cm_model *m, int32_t B, double flops[8], double *b16, double *train_f16 = nullptr) {
  CM_NOT_DIT(m, "the exec / issue FLOP split");
  if (!m || !m->finalized || !flops) return fail("model not finalized");
  for (int i = 0; i < 8; ++i) flops[i] = 0;
  if (b16) for (int i = 0; i < 8; ++i) b16[i] = 0;
  if (train_f16) for (int i = 0; i < 8; ++i) train_f16[i] = 0;
  const bool train = train_f16 != nullptr;
  // the two projections of an attention block that the plan runs as one whole-sample launch: h2 form, three 16-bit products
  // (the generic conv ops stand in for them here; q k^T and P v stay on the fp32 instruction, counted with OP_ATTN)
  std::vector<char> h2_attn(m->ops.size(), 0);
  if (!train) {
    const FwdPlan pl = plan_forward(m->ops, FwdCtx{m->precision, false, m->h2_stale, B});
    for (size_t i = 0; i < m->ops.size(); ++i)
      if (m->ops[i].kind == OP_ATTNBLK && pl.ops[i].attn_sample) h2_attn[m->ops[i].ab_qkv] = h2_attn[m->ops[i].ab_outc] = 1;
  }
  for (const Op &op : m->ops) {
    if (op.kind == OP_ATTN) { flops[op.cls] += 4.0 * op.S * (double)op.S * op.E * B; continue; }
    if (op.kind != OP_CONV) continue;
    // the inference route (the upsample convs' source statistics assumed present); `train`: the training forward's, where the
    // stand-alone skip convs run and the handle's autocast mode decides the Winograd layers' form
    const ConvRoute r = conv_route(op, m->precision, train, m->h2_stale, train && m->train_autocast);
    // 0: fp32 matrix instructions; 1: f16 operands; 6: six-term bf16 products; 3: h2 / relaxed (three cross terms)
    double mult16 = r.form == FORM_F16 ? 1.0 : r.form == FORM_B6 ? 6.0 : r.form == FORM_FP32 ? 0.0 : 3.0;
    const cm::ConvArgs &a = op.ca;
    const double Ci = a.C0 + a.C1, Cskip = op.skip0 ? op.skip0->C + (op.skip1 ? op.skip1->C : 0) : 0;   // (fused 1x1x1 skip conv)
    double f = op.flops_per_sample;
    switch (r.kernel) {
      case CONV_NONE: continue;
      case CONV_F16D:
        f = (double)(a.Zo / op.f16d_bz) * (a.Yo / op.f16d_by) * (a.Xo / op.f16d_bx) * 128.0 * op.f16d_mbw * a.Co * (Ci * 27.0 + Cskip) * 2;
        break;
      case CONV_FIN:
        // 64-row x 128-column x 32-deep GEMM per (plane, in-plane tile): rows beyond the halo box and columns beyond 27 x Co are padding
        f = (double)(a.Yo / op.fin_by) * (a.Xo / op.fin_bx) * a.Zo * 64.0 * 128.0 * 32.0 * 2;
        break;
      case CONV_QR:
        // whole 32-row blocks, one or two per plane
        f = 2.0 * (a.Yo * a.Xo > 32 ? 2 : 1) * 32 * a.Co * (Ci * 18.0 + Cskip) * 2;
        break;
      case CONV_WINO:   // per tile and 32-channel block (the fused skip conv stays fp32: counted with the layer, a few % of it)
        f = (double)a.ntz * a.nty * a.ntx * ((a.Co + 31) / 32) * (16.0 * 32 * 32 * Ci * 3 * 2 + 4.0 * 32 * 32 * Cskip * 2);
        break;
      case CONV_UPS: {
        // whole 32-row blocks per (tile, class); planes tiles that span Z skip one of 2 MBW (row block, z tap) pairs
        const double tiles = (double)(a.Zs / op.ups_tz) * (a.Ys / op.ups_ty) * (a.Xs / op.ups_tx);
        const double pairs = 2.0 * op.ups_mbw - ((op.ups_planes && op.ups_tz == a.Zs) ? 1.0 : 0.0);
        f = tiles * 8.0 * 32.0 * pairs * 4.0 * a.Co * Ci * 2;
        break;
      }
      case CONV_1X1_F16: mult16 = 0.0;   // (a 1x1x1 layer's f16 products have always been counted with the fp32 issue; kept)
      // fallthrough
      default:
        if (a.par) f = f * 8.0 / 27.0;
        // two-plane source: 6 of 8 (row block, z tap) pairs; two-plane grid: the padding-plane tap is never issued
        if (cm::conv_zsplit_variant(a, op.MB, op.NB)) f *= a.par ? 6.0 / 8.0 : 18.0 / 27.0;
    }
    if (h2_attn[&op - m->ops.data()]) mult16 = 3.0;
    if (train) { flops[op.cls] += f * B; if (r.form == FORM_F16) train_f16[op.cls] += f * B; continue; }
    if (b16 && mult16 > 0.0) b16[op.cls] += mult16 * f * B;
    else flops[op.cls] += f * B;
  }
  return 0;
}

int cm_model_exec_flops(const cm_model *m, int32_t B, double flops[8]) { return exec_flops_split(m, B, flops, nullptr); }

int cm_train_exec_flops(const cm_model *m, int32_t B, double flops[8], double f16[8]) {
  if (!f16) return fail("null output");
  return exec_flops_split(m, B, flops, nullptr, f16);
}

int cm_model_issue_flops(const cm_model *m, int32_t B, double f32[8], double b16[8]) {
  if (!b16) return fail("null output");
  return exec_flops_split(m, B, f32, b16);
}

int cm_model_class_flops(const cm_model *m, int32_t B, double flops[8]) {
  CM_NOT_DIT(m, "cm_model_class_flops");
  if (!m || !m->finalized || !flops) return fail("model not finalized");
  for (int i = 0; i < 8; ++i) flops[i] = 0;
  for (const Op &op : m->ops) {
    if (op.kind == OP_CONV) flops[op.cls] += op.flops_per_sample * B;
    else if (op.kind == OP_ATTN) flops[op.cls] += 4.0 * op.S * (double)op.S * op.E * B;
  }
  return 0;
}

}  // extern "C"

#include "cm_opt_store.inc"
#include "cm_train_host.inc"
#include "cm_dit_train_host.inc"
#include "cm_convrnn_host.inc"
#include "cm_metrics_host.inc"
