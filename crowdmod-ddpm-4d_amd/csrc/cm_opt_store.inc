// The optimizer store of the three native trainers: master weights, gradients and the Adam moments as flat fp32 buffers in
// state_dict order, the update (torch.optim.Adam with coupled L2; with `vmax`, amsgrad=True) and the accessors behind every
// family's entry points.  A frozen tensor (requires_grad False: the sinusoid tables) keeps its slot in every buffer, so that
// offsets follow the state_dict, and is left out of the update: one launch per contiguous trainable range.

namespace {

struct OptLayout {
  std::vector<size_t> off;                             // per state_dict tensor: offset in the flat buffers
  size_t nfloats = 0;
  std::vector<std::pair<size_t, size_t>> ranges;       // [begin, end) of every maximal run of trainable tensors; none is empty
};

OptLayout opt_layout(const std::vector<Param> &params, const std::vector<int> &frozen) {
  OptLayout L;
  size_t begin = 0;
  for (size_t i = 0; i < params.size(); ++i) {
    L.off.push_back(L.nfloats);
    const size_t end = L.nfloats + (size_t)params[i].numel();
    if (std::find(frozen.begin(), frozen.end(), (int)i) != frozen.end()) {
      if (L.nfloats > begin) L.ranges.push_back({begin, L.nfloats});
      begin = end;
    }
    L.nfloats = end;
  }
  if (L.nfloats > begin) L.ranges.push_back({begin, L.nfloats});
  return L;
}

struct OptStore : OptLayout {
  float *p = nullptr, *g = nullptr, *m = nullptr, *v = nullptr, *vmax = nullptr;
  float lr = 0, b1 = 0, b2 = 0, eps = 0, wd = 0;
  int step = 0;

  void hyper(float lr_, float b1_, float b2_, float eps_, float wd_) { lr = lr_; b1 = b1_; b2 = b2_; eps = eps_; wd = wd_; }

  // The buffers through the handle's allocator `alloc(float **, floats)`, zeroed; then the master weights from the device
  // copies dev_w[i] or, without them, from the host tensors.
  template <class Alloc>
  int init(const std::vector<Param> &params, const std::vector<int> &frozen, bool amsgrad, Alloc &&alloc, const float *const *dev_w = nullptr) {
    static_cast<OptLayout &>(*this) = opt_layout(params, frozen);
    for (float **b : {&p, &g, &m, &v, &vmax}) {
      if (b == &vmax && !amsgrad) break;
      if (alloc(b, nfloats)) return 1;
      CM_HIP(hipMemset(*b, 0, nfloats * sizeof(float)));
    }
    for (size_t i = 0; i < params.size(); ++i)
      CM_HIP(hipMemcpy(p + off[i], dev_w ? dev_w[i] : params[i].host.data(), (size_t)params[i].numel() * sizeof(float),
                       dev_w ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    return 0;
  }

  int apply(hipStream_t st) {
    step += 1;
    for (const auto &r : ranges)
      CM_HIP(cm::launch_adam(p + r.first, g + r.first, m + r.first, v + r.first, vmax ? vmax + r.first : nullptr,
                             (long long)(r.second - r.first), lr, b1, b2, eps, wd, step, st));
    return 0;
  }

  int find(const std::vector<Param> &params, const char *name, int64_t numel, size_t *o) const {
    if (!name) return fail("null parameter name");
    for (size_t i = 0; i < params.size(); ++i) {
      if (params[i].name != name) continue;
      if (numel != params[i].numel()) return fail("size mismatch for %s: %lld elements, got %lld", name, (long long)params[i].numel(), (long long)numel);
      *o = off[i];
      return 0;
    }
    return fail("unknown parameter %s", name);
  }

  // One tensor's slice of `buf` (p, g, m, v or vmax) to the host, or from it.  The accessors are not on the step path: they
  // wait for whatever any stream of the device still has in flight.
  int copy(const std::vector<Param> &params, float *buf, const char *name, int64_t numel, float *host, bool out) const {
    size_t o = 0;
    if (!buf || !host) return fail("null argument");
    if (find(params, name, numel, &o)) return 1;
    CM_HIP(hipDeviceSynchronize());
    if (out) CM_HIP(hipMemcpy(host, buf + o, (size_t)numel * sizeof(float), hipMemcpyDeviceToHost));
    else CM_HIP(hipMemcpy(buf + o, host, (size_t)numel * sizeof(float), hipMemcpyHostToDevice));
    return 0;
  }
  int copy_out(const std::vector<Param> &params, float *buf, const char *name, int64_t numel, float *host) const {
    return copy(params, buf, name, numel, host, true);
  }
  int copy_in(const std::vector<Param> &params, float *buf, const char *name, int64_t numel, const float *host) const {
    return copy(params, buf, name, numel, const_cast<float *>(host), false);
  }

  int opt_step(int32_t *s, int32_t set) {
    if (!s || (set && *s < 0)) return fail("optimizer step must be >= 0 (and its pointer not null)");
    if (set) step = *s;
    *s = step;
    return 0;
  }

  int flat_grads(void **d_grads, int64_t *numel) const {
    if (!d_grads || !numel) return fail("null argument");
    *d_grads = g; *numel = (int64_t)nfloats;
    return 0;
  }

  int pull_masters(std::vector<Param> &params) const {
    CM_HIP(hipDeviceSynchronize());
    for (size_t i = 0; i < params.size(); ++i)
      CM_HIP(hipMemcpy(params[i].host.data(), p + off[i], (size_t)params[i].numel() * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
  }
};

}  // namespace
