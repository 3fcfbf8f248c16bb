// Training step host orchestration (included at the end of cm_model.cpp: same translation
// unit, shares its internal types).  Mirrors DDPM_model._train_step + optimizer.step()
// (/root/reference/models/diffusion/ddpm.py:111-121,142-144): q-sample, UNet forward with
// Dropout3d, MSE, full backward, Adam with coupled L2.
//
// The backward walks the forward op list in reverse, from a plan built once (plan_backward: routes, pool regions, first writers, job
// tables; train_setup allocates what it names, backward_ops executes it).  For a conv op
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

namespace {

// One op of the backward: what runs, on which geometry, where its sums go.  No buffer of the training state appears here:
// train_setup allocates what an entry names (cm_train_state::Dgrad), the executor (backward_ops) joins the two.
enum BwdTail { TAIL_ADD, TAIL_POOL, TAIL_GN };   // the data gradient reaches the inputs by a plain accumulate / the 2x2x2 sum-pool / the GroupNorm + SiLU backward
struct BwdOp {
  int op = -1;                                   // index in the forward list; OP_CONV and OP_ATTN entries launch
  const Act *qa = nullptr, *oa = nullptr;        // OP_ATTN: the activations behind qkv (gradient written) and aout (gradient read)
  BwdGeom g;
  WgradRoute wg{WG_GENERIC, FORM_FP32};
  DgradRoute dg{DG_NONE, FORM_FP32};
  cm::ConvArgs wa{}; int wMB = 1;                // weight gradient: the geometry of its kernel's own tile
  cm::WgradPackArgs pa{}; int CN = 0;            // ... of the packed-column kernel (narrow side: 4 = mirrored, the last conv; 8 = the first)
  // partial copies of a weight-gradient launch (wgrad_groups): min(g_unit tiles per sample x B, max(g_floor, g_target / g_div) -- one
  // full round of resident workgroups, as few partial copies as that allows --, what the partial buffer holds at per_g floats each)
  int ncb = 1, nkb = 1, NKB = 1, g_target = 0, g_floor = 1, g_div = 1;
  long long g_unit = 1; size_t per_g = 1;
  BwdTail tail = TAIL_ADD;
  size_t bias_off = 0, gn_off = 0;               // batch-sum pool: [max_batch][Co] voxel sums of dY; [max_batch][2][Ctot] gamma / beta sums (TAIL_GN)
  bool acc_resid = false, acc_in0 = false, acc_in1 = false;   // the gradient buffer already holds a contribution: accumulate (else: first write)
};
struct BwdSumJob { size_t off; std::string param; int C, stride; };   // pool region, summed over the batch -> the parameter's gradient
struct BwdCopyJob { std::string param; bool bias; int off; long long n; };   // slice of the dense_1 weight / bias gradients of all blocks -> the parameter's
struct BwdPlan {
  std::vector<BwdOp> ops;                        // one per forward op, in execution (reverse) order
  size_t pool_floats = 0, attn_floats = 0;       // batch-sum pool; attention scratch at max_batch
  std::vector<BwdSumJob> bsum; std::vector<BwdCopyJob> copy;
  int bs_maxC = 0, vs_maxC = 0, nconv = 0; long long cp_max = 0;
  std::string err;                               // the list cannot run
  const BwdOp &of(size_t oi) const { return ops[ops.size() - 1 - oi]; }
};

// partial copies of entry e's weight-gradient launch at batch B; 0 (and the error text set) when the partial buffer holds none
int wgrad_groups(const BwdOp &e, int B, size_t wpart_floats) {
  const long long units = e.wg.kernel == WG_1X1 ? ((long long)B * e.g_unit + 127) / 128 : (long long)B * e.g_unit;
  const long long G = std::min<long long>(std::min<long long>(units, std::max(e.g_floor, e.g_target / e.g_div)), (long long)(wpart_floats / e.per_g));
  if (G < 1) fail("wgrad partial buffer too small");
  return (int)std::max<long long>(G, 0);
}

// the weight-gradient part of a conv entry: tile and partial-copy constants of the routed kernel
std::string plan_wgrad(const Op &op, const BwdKnobs &k, BwdOp &e) {
  const int Co = op.ca.Co;
  cm::ConvArgs &wa = e.wa;
  wa = e.g.wa; e.wMB = e.g.wMB;
  e.ncb = (Co + 31) / 32; e.nkb = (wa.C0 + wa.C1 + 31) / 32;
  const int nn = e.ncb * e.nkb;
  auto tiles = [&] { return (long long)wa.ntz * wa.nty * wa.ntx; };
  switch (e.wg.kernel) {
    case WG_WINO:
      wa = op.ca; wa.bs = 1; wa.ks = 1;
      if (!cm::conv_wino_pick(wa.Zo, wa.Yo, wa.Xo, &wa.bz, &wa.by, &wa.bx)) return "no Winograd tile for the weight gradient of " + op.label;
      wa.ntz = wa.Zo / wa.bz; wa.nty = (wa.Yo + wa.by - 1) / wa.by; wa.ntx = (wa.Xo + wa.bx - 1) / wa.bx;
      e.g_unit = tiles(); e.per_g = (size_t)nn * 48 * 1024; e.g_target = k.wino_wgs; e.g_floor = 1; e.g_div = nn;
      break;
    case WG_PACK: {
      cm::WgradPackArgs &pa = e.pa;
      pa.mirror = Co <= 4; e.CN = pa.mirror ? 4 : 8; pa.cn_valid = pa.mirror ? Co : e.g.Ci;
      pa.Z = op.ca.Zo; pa.Y = op.ca.Yo; pa.X = op.ca.Xo;
      pa.bz = std::min(pa.Z, 8); pa.by = std::min(pa.Y, 4); pa.bx = std::min(pa.X, 6);
      if ((pa.bz * pa.by * pa.bx) & 1) pa.bx += 1;   // (an even number of rows: voxel pairs; rows outside the grid are zero)
      pa.ntz = (pa.Z + pa.bz - 1) / pa.bz; pa.nty = (pa.Y + pa.by - 1) / pa.by; pa.ntx = (pa.X + pa.bx - 1) / pa.bx;
      e.g_unit = (long long)pa.ntz * pa.nty * pa.ntx; e.per_g = (size_t)((27 * e.CN + 31) / 32) * 1024; e.g_target = 256;
      break;
    }
    case WG_PAR:
      wa.bz = std::min(wa.Zs, 4); wa.by = std::min(wa.Ys, 6); wa.bx = std::min(wa.Xs, wa.Zs <= 2 ? 9 : 6);
      wa.ntz = (wa.Zs + wa.bz - 1) / wa.bz; wa.nty = (wa.Ys + wa.by - 1) / wa.by; wa.ntx = (wa.Xs + wa.bx - 1) / wa.bx;
      e.g_unit = tiles(); e.per_g = (size_t)nn * 64 * 1024; e.g_target = k.par_wgs; e.g_floor = 2; e.g_div = 8 * nn;
      break;
    case WG_1X1:
      e.NKB = e.nkb % 4 == 0 ? 4 : (e.nkb % 3 == 0 ? 3 : (e.nkb % 2 == 0 ? 2 : 1));
      e.g_unit = op.out_act->V(); e.per_g = (size_t)nn * 1024; e.g_target = k.x1_wgs; e.g_floor = 4; e.g_div = e.ncb * (e.nkb / e.NKB);
      break;
    case WG_ZS: case WG_GENERIC:
      if (e.g.zsplit) { wa.zsplit = 1; e.wMB = 2; }
      e.g_unit = tiles(); e.g_floor = 4;
      e.per_g = (size_t)nn * (wa.par ? 64 : (op.ref_taps == 1 ? 4 : op.ref_taps)) * 1024;   // parity form: 8 classes x 8 taps per group; 1x1x1: 4 per-wave partials
      if (e.wg.kernel == WG_ZS) { e.g_target = k.zs_wgs; e.g_div = e.ncb * ((e.nkb + 1) / 2); }   // two input blocks per workgroup
      else { e.g_target = k.wgs; e.g_div = nn; }
      break;
  }
  return "";
}

// The backward sibling of plan_forward: everything the backward's launches depend on, decided in one walk over the op list in
// reverse -- each conv's two routes (wgrad_route, dgrad_route), the partial-copy constants, every region of the batch-sum pool, who
// writes each gradient buffer first, the job tables of the deferred sums.  Pure: allocates nothing, launches nothing.
BwdPlan plan_backward(const std::vector<Op> &ops, const BwdCtx &ctx, const BwdKnobs &k) {
  BwdPlan P;
  std::map<const Act *, int> have{{ctx.seed, -1}};   // gradient buffers that hold a contribution so far -> the forward op that wrote first (-1: the loss gradient)
  auto first_write = [&](const Act *a, int oi) { return have.emplace(a, oi).second; };
  for (int oi = (int)ops.size() - 1; oi >= 0 && P.err.empty(); --oi) {
    const Op &op = ops[oi];
    P.ops.emplace_back();
    BwdOp &e = P.ops.back();
    e.op = oi;
    if (op.kind == OP_ATTN) {
      // qkv is the op's input tensor, aout its output: their activations are the neighbouring convs' output / source
      for (const Op &o : ops) {
        if (o.kind == OP_CONV && o.out_act->d == op.qkv) e.qa = o.out_act;
        if (o.kind == OP_CONV && o.in0->d == op.aout) e.oa = o.in0;
      }
      if (!e.qa || !e.oa || !have.count(e.oa)) { P.err = "attention backward: missing gradient (" + op.label + ")"; break; }
      if (const char *why = cm::attn_bwd_limit(op.S, op.E, ATTN_HEADS)) {
        P.err = "training refused: " + op.label + " (" + std::to_string(op.S) + " tokens, " + std::to_string(op.E / ATTN_HEADS) + " channels per head): " + why;
        break;
      }
      P.attn_floats = std::max(P.attn_floats, cm::attn_bwd_scratch_floats(ctx.max_batch, op.S, op.E, ATTN_HEADS));
      have.emplace(e.qa, oi);
      continue;
    }
    if (op.kind != OP_CONV) continue;
    if (!have.count(op.out_act)) { P.err = "backward: no gradient reached " + op.label; break; }
    ++P.nconv;
    const int Co = op.ca.Co, Ctot = op.ca.C0 + op.ca.C1;
    e.g = bwd_geom(op, ctx, k);
    e.wg = wgrad_route(op, e.g, ctx, k);
    e.dg = dgrad_route(op, e.g, ctx, k);
    if (op.resid_act) e.acc_resid = !first_write(op.resid_act, oi);
    // bias gradient and the broadcast time-embedding term: voxel sums of dY, which stays intact until the end of the pass (every
    // act owns its buffer and all of its consumers have already contributed)
    e.bias_off = P.pool_floats; P.pool_floats += (size_t)ctx.max_batch * Co;
    P.bsum.push_back({e.bias_off, op.bname, Co, Co});
    P.vs_maxC = std::max(P.vs_maxC, Co); P.bs_maxC = std::max(P.bs_maxC, Co);
    P.err = plan_wgrad(op, k, e);
    if (e.dg.kernel == DG_NONE || !P.err.empty()) continue;
    if (dgrad_wino_ok(e.g, k) && !cm::conv_wino_ok(e.g.da)) P.err = "Winograd data-gradient tile does not fit " + op.label;
    if (e.dg.kernel == DG_QR) {
      static float set;
      cm::QrArgs q{};
      q.C0 = e.g.da.C0; q.raw = 1; q.groups = 8; q.wq6 = &set; q.out_cs = e.g.da.out_cs; q.Co = e.g.da.Co; q.Y = e.g.da.Yo; q.X = e.g.da.Xo;
      if (!cm::conv_qr2_b6_ok(q)) P.err = "quarter-resolution data gradient of " + op.label + ": no six-term form";
    }
    e.tail = op.ca.par ? TAIL_POOL : op.gn_op >= 0 ? TAIL_GN : TAIL_ADD;
    if (e.tail == TAIL_GN) {
      const Op &gop = ops[op.gn_op];
      e.gn_off = P.pool_floats; P.pool_floats += (size_t)ctx.max_batch * 2 * Ctot;
      P.bsum.push_back({e.gn_off, gop.gname, Ctot, 2 * Ctot});
      P.bsum.push_back({e.gn_off + Ctot, gop.bename, Ctot, 2 * Ctot});
      P.bs_maxC = std::max(P.bs_maxC, Ctot);
      e.acc_in1 = op.in1 && have.count(op.in1);
    }
    e.acc_in0 = !first_write(op.in0, oi);
    if (op.in1 && e.tail != TAIL_POOL) { const bool fw = first_write(op.in1, oi); if (e.tail == TAIL_ADD) e.acc_in1 = !fw; }
  }
  // the per-block slices of the time-projection gradients -> their parameters' slots (conv_1 of every ResnetBlock, forward order)
  for (const Op &op : ops)
    if (op.kind == OP_CONV && op.temb_off >= 0) {
      const std::string prefix = op.wname.substr(0, op.wname.size() - std::string(".conv_1.weight").size());
      P.copy.push_back({prefix + ".dense_1.weight", false, op.temb_off, (long long)op.ca.Co * ctx.tx});
      P.copy.push_back({prefix + ".dense_1.bias", true, op.temb_off, (long long)op.ca.Co});
      P.cp_max = std::max(P.cp_max, (long long)op.ca.Co * ctx.tx);
    }
  return P;
}

// The plan as text, one line per launching entry in execution (reverse) order:
//   conv <label> wgrad <kernel> <form> dgrad <kernel> <form>
//   attn <label> S <tokens> D <channels per head> <lds | slab>     (where P and dS of a (sample, head) live)
// Reads the plan and the op list only.
const char *const kWgradName[] = {"WG_WINO", "WG_PACK", "WG_PAR", "WG_1X1", "WG_ZS", "WG_GENERIC"};
const char *const kDgradName[] = {"DG_NONE", "DG_QR", "DG_WINO", "DG_GENERIC"};
const char *form_name(ConvForm f) {
  switch (f) { case FORM_FP32: return "fp32"; case FORM_B6: return "b6"; case FORM_B3: return "b3"; case FORM_H2: return "h2"; case FORM_F16: return "f16"; }
  return "?";
}
std::string bwd_plan_text(const std::vector<Op> &ops, const BwdPlan &P, int max_batch) {
  std::string out;
  for (const BwdOp &e : P.ops) {
    const Op &op = ops[e.op];
    if (op.kind == OP_ATTN)
      out += "attn " + op.label + " S " + std::to_string(op.S) + " D " + std::to_string(op.E / ATTN_HEADS) +
             (cm::attn_bwd_scratch_floats(max_batch, op.S, op.E, ATTN_HEADS) ? " slab\n" : " lds\n");
    if (op.kind == OP_CONV)
      out += "conv " + op.label + " wgrad " + kWgradName[e.wg.kernel] + " " + form_name(e.wg.form) + " dgrad " + kDgradName[e.dg.kernel] + " " +
             form_name(e.dg.form) + "\n";
  }
  return out;
}

}  // namespace

struct cm_train_state {
  BwdKnobs knobs;             // the backward's diagnostic switches, read once (cm_train_init)
  BwdPlan bwd;                 // what the backward launches, decided once from the op list (plan_backward)
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
  // per conv op: the device buffers its plan entry (BwdOp) names
  struct Dgrad {
    int *d_hv = nullptr, *d_mt = nullptr;   // data gradient on the generic kernel: coordinate tables, fragments, a zero bias
    float *wfrag = nullptr, *zero_bias = nullptr;
    float *wwino = nullptr;     // ... on the Winograd kernel (cm_conv_wino.hip): transformed weights
    float *wwino_b6 = nullptr;  // six-term bf16 split of wwino (pack_wino_b6 order), re-derived after every optimizer step
    long long wwino_floats = 0;
    float *wwino16 = nullptr;   // autocast: f16 sibling of wwino_b6 (pack_wino_f16 order), allocated when mode 1 is first set
    // two-plane grids: the data gradient on the whole-sample kernel conv_qr2 in its six-term form (no normalisation: `raw`)
    float *wqr = nullptr, *wqr_b6 = nullptr;
    long long wqr_floats = 0; int wqr_C0 = 0;   // (C0: the input channels of the data gradient = Cy)
    int *w_hv = nullptr, *w_mt = nullptr;   // weight gradient: coordinate tables of its own tile
  };
  std::vector<Dgrad> dg;  // indexed like m->ops
  // scratch
  float *scrA = nullptr, *scrB = nullptr, *scrC = nullptr;  // [B][Vfull][Cmax]
  float *wpart = nullptr; size_t wpart_floats = 0;
  float *tmp_bc = nullptr;       // [B][Cmax]
  cm::CopyJob *d_cp_jobs = nullptr;
  float *attn_big = nullptr;     // S x S scratch of the attention backward at large token counts (BwdPlan::attn_floats)
  // deferred batch reductions: every conv / GroupNorm of the backward pass leaves its per-sample sums in its own region
  // of bs_pool; one job-table launch at the end turns them into the parameter gradients (the plan fixes the regions and the
  // jobs, train_setup uploads the tables: only B, a launch argument, changes between steps)
  float *bs_pool = nullptr;
  cm::BsumJob *d_bs_jobs = nullptr;
  cm::VsumJob *d_vs_jobs = nullptr;   // the per-sample voxel sums feeding them, deferred the same way
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

int upload_ints(cm_model *m, const std::vector<int> &h, int **d) {
  if (dev_alloc(m, (void **)d, h.size() * sizeof(int))) return 1;
  CM_HIP(hipMemcpy(*d, h.data(), h.size() * sizeof(int), hipMemcpyHostToDevice));
  return 0;
}
// the box coordinate tables of a tile the plan picked (tune_tile)
int upload_tables(cm_model *m, const cm::ConvArgs &ca, int MB, int **d_hv, int **d_mt) {
  std::vector<int> hv((size_t)cm::conv_halo_voxels(ca)), mt((size_t)32 * MB);
  cm::conv_build_tables(ca, MB, hv.data(), mt.data());
  return upload_ints(m, hv, d_hv) || upload_ints(m, mt, d_mt);
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

// the loss-scale exponent of an autocast step over N loss elements (UNet and DiT4D trainers): the requested one, or the largest k
// with 2^k <= N (loss gradient O(1))
int loss_scale_log2(int ls_req, long long N) {
  int k = 0;
  while (k < 24 && (2LL << k) <= N) ++k;
  return ls_req >= 0 ? ls_req : k;
}
int autocast_scale_log2(const cm_model *m, int B) {
  const cm_unet_config &c = m->cfg;
  return loss_scale_log2(m->train->ls_req, (long long)B * c.out_channels * c.rows * c.cols * c.future_len);
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
    if (D.wqr_b6) CM_HIP(cm::launch_qr_b6_repack(D.wqr, D.wqr_b6, D.wqr_floats, D.wqr_C0, st));
  }
  return T->autocast ? repack_f16(m, st) : 0;
}

BwdCtx bwd_ctx(const cm_model *m) {
  BwdCtx x;
  x.precision = m->precision; x.max_batch = m->cfg.max_batch; x.in_channels = m->cfg.in_channels;
  x.tx = m->cfg.base_channels * m->cfg.time_multiple; x.x8 = m->x8_act; x.seed = m->act_by_name.at("final");   // (written by mse_grad)
  if (m->train) { x.autocast = m->train->autocast != 0; x.f16_frags = m->train->ac_ready; }
  return x;
}

// The plan first; then the buffers it names, in forward op order (the order of `derived` / `derived_wino` is that of the re-pack
// job tables, which cm_train_set_autocast checks).
int train_setup(cm_model *m) {
  cm_train_state *T = m->train;
  const cm_unet_config &c = m->cfg;
  const size_t B = (size_t)c.max_batch;
  T->knobs = read_bwd_knobs();
  T->bwd = plan_backward(m->ops, bwd_ctx(m), T->knobs);
  if (!T->bwd.err.empty()) return fail("%s", T->bwd.err.c_str());
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
  if (dev_alloc(m, (void **)&T->bs_pool, T->bwd.pool_floats * sizeof(float))) return 1;
  if (T->bwd.attn_floats && dev_alloc(m, (void **)&T->attn_big, T->bwd.attn_floats * sizeof(float))) return 1;
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
    // ---- what the op's plan entry names: fragments and tables of its data gradient (BwdGeom::da), tables of its weight gradient ----
    cm_train_state::Dgrad &D = T->dg[oi];
    const BwdOp &e = T->bwd.of(oi);
    const BwdGeom &g = e.g;
    op.train_qr = e.dg.kernel == DG_QR;              // the training forward takes conv_qr2 where the data gradient does (conv_route)
    if (!g.first) {
      const int Cy = g.da.C0;
      std::vector<int> src((size_t)Ci * Co * nt);    // W'[ci][co][t'] = W[co][ci][flip t']
      for (int ci = 0; ci < Ci; ++ci)
        for (int co = 0; co < Co; ++co)
          for (int t = 0; t < nt; ++t) src[((size_t)ci * Co + co) * nt + t] = ii[((size_t)co * Ci + ci) * nt + (nt - 1 - t)];
      const std::vector<int> pidx = pack_conv(src.data(), Ci, Co, nt, Cy, g.da.CK, g.dNB, -1);
      if (dev_alloc(m, (void **)&D.wfrag, pidx.size() * sizeof(float))) return 1;
      if (add_derived(m, D.wfrag, pidx, 1, true)) return 1;
      const int TN = 32 * g.dNB, cop = (Ci + TN - 1) / TN * TN;
      std::vector<float> zb((size_t)cop, 0.f);
      if (upload(m, zb, &D.zero_bias)) return 1;
      if (dgrad_wino_ok(g, T->knobs)) {
        // the Winograd kernel's transformed weights, re-derived from the master copy after every update, and their six-term split
        const size_t nel = (size_t)((Ci + 31) / 32) * (Cy / 16) * 4 * 24 * 64 * 4;
        if (dev_alloc(m, (void **)&D.wwino, nel * sizeof(float))) return 1;
        if (add_derived_wino(m, D.wwino, src, Ci, Co, Cy)) return 1;
        D.wwino_floats = (long long)nel;
        if (dgrad_wino_b6(g, bwd_ctx(m), T->knobs) && dev_alloc(m, (void **)&D.wwino_b6, nel * 3 / 2 * sizeof(float))) return 1;
      } else if (upload_tables(m, g.da, g.dMB, &D.d_hv, &D.d_mt)) return 1;
      if (e.dg.kernel == DG_QR) {
        const int ntn = Ci / 32, cw = Co / 8, nsw = (cw + 15) >> 4;
        const std::vector<int> wq = pack_qr(src, Ci, Co);                 // dgrad output channels Ci, input channels Co (= Cy)
        D.wqr_floats = (long long)wq.size(); D.wqr_C0 = Cy;
        if (dev_alloc(m, (void **)&D.wqr, wq.size() * sizeof(float))) return 1;
        if (add_derived(m, D.wqr, wq, 1, true)) return 1;
        const size_t n6 = (size_t)ntn * 8 * nsw * 9 * 3 * 3 * 64 * 4;      // pack_qr_b6 order, padded steps stay zero
        if (dev_alloc(m, (void **)&D.wqr_b6, n6 * sizeof(float))) return 1;
        CM_HIP(hipMemset(D.wqr_b6, 0, n6 * sizeof(float)));
      }
    }
    if (upload_tables(m, g.wa, g.wMB, &D.w_hv, &D.w_mt)) return 1;
    if (g.zsplit) {
      std::vector<int> mt(64, -1);
      for (int z = 0; z < 2; ++z)
        for (int y = 0; y < g.wa.by; ++y)
          for (int x = 0; x < g.wa.bx; ++x) mt[(size_t)z * 32 + y * g.wa.bx + x] = (z << 18) | (y << 9) | x;
      if (upload_ints(m, mt, &D.w_mt)) return 1;
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
  // the plan's job tables of the deferred sums, as device tables
  {
    std::vector<cm::VsumJob> vs; std::vector<cm::BsumJob> bs; std::vector<cm::CopyJob> cp;
    for (const BwdOp &e : T->bwd.ops) {
      const Op &op = m->ops[e.op];
      if (op.kind != OP_CONV) continue;
      const int Co = op.ca.Co;
      vs.push_back({op.out_act->g, op.out_act->V(), Co, op.out_act->C, T->bs_pool + e.bias_off, Co, op.temb_off >= 0 ? T->dproj + op.temb_off : nullptr, m->nproj});
    }
    for (const BwdSumJob &j : T->bwd.bsum) bs.push_back({T->bs_pool + j.off, grad_of(m, j.param), j.C, j.stride});
    for (const BwdCopyJob &j : T->bwd.copy)
      cp.push_back({grad_of(m, j.param), j.bias ? T->dbd_all + j.off : T->dWd_all + (size_t)j.off * tx, j.n});
    if (dev_alloc(m, (void **)&T->d_vs_jobs, vs.size() * sizeof(cm::VsumJob)) || dev_alloc(m, (void **)&T->d_bs_jobs, bs.size() * sizeof(cm::BsumJob)) ||
        dev_alloc(m, (void **)&T->d_cp_jobs, cp.size() * sizeof(cm::CopyJob))) return 1;
    CM_HIP(hipMemcpy(T->d_vs_jobs, vs.data(), vs.size() * sizeof(cm::VsumJob), hipMemcpyHostToDevice));
    CM_HIP(hipMemcpy(T->d_bs_jobs, bs.data(), bs.size() * sizeof(cm::BsumJob), hipMemcpyHostToDevice));
    CM_HIP(hipMemcpy(T->d_cp_jobs, cp.data(), cp.size() * sizeof(cm::CopyJob), hipMemcpyHostToDevice));
  }
  // every derived tensor (forward fragments included) is rebuilt from the master copy by the same
  // kernel that re-packs after an optimizer step, so a handle resumed from a checkpoint continues
  // bit-identically to the handle that wrote it
  if (repack_all(m, m->stream)) return 1;
  CM_HIP(hipDeviceSynchronize());
  return 0;
}

// accumulate a channels-last gradient slice into an activation's gradient buffer (acc = 0: first write)
int accum_act(const Act *a, const float *src, int src_cs, int B, bool acc, hipStream_t st) {
  CM_HIP(cm::launch_add_into(a->g, a->C, src, src_cs, a->C, (long long)B * a->V(), acc ? 1 : 0, st));
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

// The weight gradient of one conv entry on the kernel its route names, into the parameter's gradient.  Inputs: dY and forward activations.
int run_wgrad(cm_model *m, const BwdOp &e, int B, hipStream_t wst) {
  cm_train_state *T = m->train;
  const Op &op = m->ops[e.op];
  const cm_train_state::Dgrad &D = T->dg[e.op];
  const float *dY = op.out_act->g;
  const int Cy = op.out_act->C, ncb = e.ncb, nkb = e.nkb;
  float *dW = grad_of(m, op.wname);
  const int G = wgrad_groups(e, B, T->wpart_floats);
  if (G < 1) return 1;
  cm::ConvArgs wa = e.wa;
  wa.B = B;
  if (op.pm_off >= 0) { wa.pm = m->dropmask + op.pm_off; wa.pm_stride = m->nproj; }
  if (e.wg.kernel != WG_WINO) { wa.hvtab = D.w_hv; wa.mtab = D.w_mt; }
  switch (e.wg.kernel) {
    case WG_WINO:
      if (e.wg.form == FORM_F16) CM_HIP(cm::launch_wgrad_wino_f16(wa, dY, Cy, T->wpart, G, ncb, nkb, wst));
      else CM_HIP(cm::launch_wgrad_wino(wa, dY, Cy, T->wpart, G, ncb, nkb, wst));
      CM_HIP(cm::launch_wgrad_wino_reduce(T->wpart, G, ncb, nkb, e.g.Co, e.g.Ci, dW, wst));
      break;
    case WG_PACK: {
      cm::WgradPackArgs pa = e.pa;
      if (pa.mirror) {
        pa.wide = op.in0->d; pa.wide_cs = op.in0->C; pa.gn = op.ca.gn; pa.silu = op.ca.silu;
        pa.narrow = dY; pa.narrow_cs = Cy;
      } else {
        pa.wide = dY; pa.wide_cs = Cy; pa.gn = nullptr; pa.silu = 0;
        pa.narrow = op.in0->d; pa.narrow_cs = op.in0->C;
      }
      pa.B = B; pa.part = T->wpart;
      CM_HIP(cm::launch_wgrad_pack(pa, e.CN, G, wst));
      CM_HIP(cm::launch_wgrad_pack_reduce(T->wpart, G, e.CN, pa.cn_valid, pa.mirror, e.g.Co, e.g.Ci, dW, wst));
      break;
    }
    case WG_PAR:
      CM_HIP(cm::launch_wgrad_par(wa, dY, Cy, T->wpart, G, ncb, nkb, wst));
      CM_HIP(cm::launch_wgrad_reduce_par(T->wpart, G, ncb, nkb, e.g.Co, e.g.Ci, dW, wst));
      break;
    case WG_1X1:
      CM_HIP(cm::launch_wgrad_1x1(wa, dY, Cy, op.out_act->V(), T->wpart, G, ncb, nkb, e.NKB, wst));
      CM_HIP(cm::launch_wgrad_reduce(T->wpart, G, ncb, nkb, 1, e.g.Co, e.g.Ci, dW, wst, 1));
      break;
    case WG_ZS:
      wa.nts = B;
      CM_HIP(cm::launch_wgrad_zs(wa, dY, Cy, T->wpart, G, ncb, nkb, wst));
      CM_HIP(cm::launch_wgrad_reduce(T->wpart, G, ncb, nkb, op.ref_taps, e.g.Co, e.g.Ci, dW, wst));
      break;
    case WG_GENERIC:
      wa.nts = B;
      CM_HIP(cm::launch_wgrad(wa, e.wMB, dY, Cy, T->wpart, G, ncb, nkb, wst));
      if (wa.par) CM_HIP(cm::launch_wgrad_reduce_par(T->wpart, G, ncb, nkb, e.g.Co, e.g.Ci, dW, wst));
      else CM_HIP(cm::launch_wgrad_reduce(T->wpart, G, ncb, nkb, op.ref_taps, e.g.Co, e.g.Ci, dW, wst));
      break;
  }
  return 0;
}

// The data gradient of one conv entry into scrA [B][Vin][Ctot], then on to the inputs' gradient buffers (BwdTail).
int run_dgrad(cm_model *m, const BwdOp &e, int B, hipStream_t st) {
  cm_train_state *T = m->train;
  const Op &op = m->ops[e.op];
  const cm_train_state::Dgrad &D = T->dg[e.op];
  const float *dysrc = op.out_act->g;
  const int Cy = op.out_act->C, Ctot = op.ca.C0 + op.ca.C1;
  cm::ConvArgs da = e.g.da;
  da.B = B; da.nts = (B + da.bs - 1) / da.bs;
  da.wfrag = D.wfrag; da.bias = D.zero_bias; da.hvtab = D.d_hv; da.mtab = D.d_mt;
  if (op.ca.stride == 2) {
    CM_HIP(cm::launch_zero_stuff2(dysrc, T->scrB, B, op.ca.Zo, op.ca.Yo, op.ca.Xo, Cy, st));
    dysrc = T->scrB;
  }
  da.src0 = dysrc; da.out = T->scrA; da.tidx = m->tbuf;
  switch (e.dg.kernel) {
    case DG_QR: {
      cm::QrArgs q{};
      q.src0 = dysrc; q.C0 = da.C0; q.raw = 1; q.groups = 8;
      q.wq = D.wqr; q.wq6 = D.wqr_b6; q.bias = D.zero_bias; q.tidx = m->tbuf;
      q.out = T->scrA; q.out_cs = da.out_cs; q.Co = da.Co; q.B = B; q.Y = da.Yo; q.X = da.Xo;
      CM_HIP(cm::launch_conv_qr(q, st));
      break;
    }
    case DG_WINO:
      da.wfrag = e.dg.form == FORM_F16 ? D.wwino16 : e.dg.form == FORM_B6 ? D.wwino_b6 : D.wwino;
      if (e.dg.form == FORM_B6) da.f16 = 2;
      CM_HIP(cm::launch_conv_wino(da, e.dg.form == FORM_F16, st));
      break;
    default:
      CM_HIP(cm::launch_conv(da, e.g.dMB, e.g.dNB, st));
  }
  switch (e.tail) {
    case TAIL_POOL:
      CM_HIP(cm::launch_sumpool2(T->scrA, op.in0->g, B, op.ca.Zs, op.ca.Ys, op.ca.Xs, op.in0->C, e.acc_in0 ? 1 : 0, st));
      break;
    case TAIL_GN: {
      const Op &gop = m->ops[op.gn_op];
      cm::GnbArgs ga{};
      ga.x0 = op.in0->d; ga.x1 = op.in1 ? op.in1->d : nullptr; ga.C0 = op.ca.C0; ga.C1 = op.ca.C1;
      ga.dA = T->scrA; ga.dA_cs = Ctot;
      ga.gn = gop.gn_out; ga.mr = gop.gn_mr; ga.gamma = gop.gamma;
      ga.pm = op.pm_off >= 0 ? m->dropmask + op.pm_off : nullptr; ga.pm_stride = m->nproj;
      ga.silu = op.ca.silu;
      ga.V = op.in0->V(); ga.B = B; ga.groups = GN_GROUPS;
      ga.nsl = std::max(1, std::min(MAX_SLICES, ga.V / 128));
      ga.part = T->gnb_part; ga.coef = T->gnb_coef; ga.dgb = T->bs_pool + e.gn_off;
      ga.g1 = op.in1 ? op.in1->g : nullptr; ga.acc1 = e.acc_in1 ? 1 : 0;
      ga.g0 = op.in0->g; ga.acc0 = e.acc_in0 ? 1 : 0;
      CM_HIP(cm::launch_gn_backward(ga, st));
      break;
    }
    case TAIL_ADD:
      if (accum_act(op.in0, T->scrA, Ctot, B, e.acc_in0, st)) return 1;
      if (op.in1 && accum_act(op.in1, T->scrA + op.ca.C0, Ctot, B, e.acc_in1, st)) return 1;
  }
  return 0;
}

// The executor of T->bwd: one pass over its entries.  Weight gradients are off the critical path (only the optimizer reads them), so
// their launches go to a second stream and fill the tails / launch gaps of the data-gradient chain; their inputs are dY (final: every
// consumer of the op's output has already contributed, and nothing writes it again in this pass) and forward activations, their
// outputs the parameter's gradient and the partial buffer, which only that stream touches.
int backward_ops_impl(cm_model *m, int B, hipStream_t st) {
  cm_train_state *T = m->train;
  const BwdPlan &P = T->bwd;
  CM_HIP(hipMemsetAsync(T->dproj, 0, (size_t)B * m->nproj * sizeof(float), st));
  hipStream_t wst = (T->knobs.wgrad_one_stream || !m->lane_stream[1]) ? st : m->lane_stream[1];
  if (wst != st && !T->ev_dy) {
    CM_HIP(hipEventCreateWithFlags(&T->ev_dy, hipEventDisableTiming));
    CM_HIP(hipEventCreateWithFlags(&T->ev_wdone, hipEventDisableTiming));
  }
  static const bool sync_ops = cm::diag_env("CM_SYNC_OPS") != nullptr;   // debugging: name every op and drain the device after it
  for (const BwdOp &e : P.ops) {
    const Op &op = m->ops[e.op];
    if (sync_ops) {
      const hipError_t err = hipDeviceSynchronize();
      fprintf(stderr, "[cm] backward reaches op %d %s (%s)\n", e.op, op.label.c_str(), hipGetErrorString(err));
      fflush(stderr);
    }
    if (op.kind == OP_ATTN)   // (large token counts only: the S x S matrices go to a global slab)
      CM_HIP(cm::launch_attn_bwd(op.qkv, e.oa->g, e.qa->g, B, op.S, op.E, ATTN_HEADS,
                                 cm::attn_bwd_scratch_floats(m->cfg.max_batch, op.S, op.E, ATTN_HEADS) ? T->attn_big : nullptr, st));
    if (op.kind != OP_CONV) continue;
    if (op.resid_act && accum_act(op.resid_act, op.out_act->g, op.out_act->C, B, e.acc_resid, st)) return 1;
    if (wst != st) {
      CM_HIP(hipEventRecord(T->ev_dy, st));
      CM_HIP(hipStreamWaitEvent(wst, T->ev_dy, 0));
    }
    if (run_wgrad(m, e, B, wst)) return 1;
    if (e.dg.kernel != DG_NONE && run_dgrad(m, e, B, st)) return 1;   // (the first conv: its input is data)
  }
  if (wst != st) {                                 // every weight gradient is complete before the optimizer reads it
    CM_HIP(hipEventRecord(T->ev_wdone, wst));
    CM_HIP(hipStreamWaitEvent(st, T->ev_wdone, 0));
  }
  // the deferred voxel and batch reductions (bias, time-row, gamma, beta gradients): one job-table launch each
  CM_HIP(cm::launch_voxel_sum_jobs(T->d_vs_jobs, P.nconv, B, P.vs_maxC, st));
  CM_HIP(cm::launch_batch_sum_jobs(T->d_bs_jobs, (int)P.bsum.size(), B, P.bs_maxC, st));
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
  CM_HIP(cm::launch_copy_jobs(T->d_cp_jobs, (int)P.copy.size(), P.cp_max, st));   // the per-block slices -> their parameters' gradient slots
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
    if (train_setup(m)) {     // refused (the plan's limits, memory): the handle goes on as the inference handle it was
      cm_free_train_state(m->train);
      m->train = nullptr;
      return 1;
    }
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
        if (D.wwino && dev_alloc(m, (void **)&D.wwino16, (size_t)D.wwino_floats / 2 * sizeof(float))) return 1;
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
  T->bwd = plan_backward(m->ops, bwd_ctx(m), T->knobs);   // the f16 forms of the Winograd layers' two gradients come and go with the mode
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

int cm_debug_bwd_plan(const cm_model *m, char *buf, int64_t capacity, int64_t *needed) {
  CM_NOT_DIT(m, "cm_debug_bwd_plan");
  if (!m || !needed || capacity < 0 || (capacity > 0 && !buf)) return fail("cm_debug_bwd_plan: bad argument");
  if (!m->train) return fail("cm_debug_bwd_plan: cm_train_init has not been called");
  const std::string text = bwd_plan_text(m->ops, m->train->bwd, m->cfg.max_batch);
  *needed = (int64_t)text.size() + 1;
  if (capacity > 0) snprintf(buf, (size_t)capacity, "%s", text.c_str());
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
