// C-ABI entry points of the SSIM, energy and motion-feature metric tables (kernels: cm_metrics.hip).  Every argument check
// comes before the first device call; results are float64 arrays the host owns, as with cm_frame_metrics.

namespace {

// Device scratch of one entry point, released on every return path.
struct DevScratch {
  void *p = nullptr;
  ~DevScratch() { if (p) hipFree(p); }
  hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes); }
};

int metric_shape_ok(const char *what, int32_t N, int32_t Cc, int32_t H, int32_t W, int32_t F, const char *last = "F") {
  if (N < 1) return fail("%s: N = %d must be >= 1", what, N);
  if (Cc < 1) return fail("%s: C = %d must be >= 1", what, Cc);
  if (H < 1) return fail("%s: H = %d must be >= 1", what, H);
  if (W < 1) return fail("%s: W = %d must be >= 1", what, W);
  if (F < 1) return fail("%s: %s = %d must be >= 1", what, last, F);
  return 0;
}

int motion_feature_args_ok(const char *what, int32_t N, int32_t Cc, int32_t H, int32_t W, int32_t F, int32_t f, int32_t k,
                           long long *nvol) {
  if (metric_shape_ok(what, N, Cc, H, W, F)) return 1;
  if (Cc < 3) return fail("%s: C = %d: the motion features read channels 1 and 2 (v_x, v_y), C must be >= 3", what, Cc);
  if (f < 1) return fail("%s: f = %d must be >= 1", what, f);
  if (k < 1) return fail("%s: k = %d must be >= 1", what, k);
  *nvol = cm::motion_feature_volumes(H, W, F, f, k);
  if (*nvol > 0x7fffffffLL) return fail("%s: %lld volumes per sequence exceed 2^31 - 1", what, *nvol);
  return 0;
}

}  // namespace

extern "C" {

int cm_ssim_frames(int32_t device, const float *d_pred, const float *d_gt, int32_t N, int32_t Cc, int32_t H, int32_t W,
                   int32_t F, const double *h_range, double *h_out) {
  if (!d_pred) return fail("cm_ssim_frames: d_pred is null");
  if (!d_gt) return fail("cm_ssim_frames: d_gt is null");
  if (!h_range) return fail("cm_ssim_frames: h_range is null");
  if (!h_out) return fail("cm_ssim_frames: h_out is null");
  if (metric_shape_ok("cm_ssim_frames", N, Cc, H, W, F)) return 1;
  if (std::min(H, W) < 7) return fail("cm_ssim_frames: min(H, W) = %d: SSIM needs images of at least 7x7 (got %d x %d)", std::min(H, W), H, W);
  if (!cm::ssim_frames_ok(W, F))
    return fail("cm_ssim_frames: W * F = %lld above %d (one row of the LDS band holds at most 128 columns x 8 frames)", (long long)W * F, cm::kSsimMaxRow);
  if ((long long)N * Cc > 0x7fffffffLL) return fail("cm_ssim_frames: N * C = %lld exceeds 2^31 - 1", (long long)N * Cc);
  DevGuard g(device);
  const size_t cells = (size_t)N * Cc * F;
  DevScratch out, rng;
  CM_HIP(out.alloc(cells * sizeof(double)));
  CM_HIP(rng.alloc((size_t)Cc * sizeof(double)));
  CM_HIP(hipMemcpy(rng.p, h_range, (size_t)Cc * sizeof(double), hipMemcpyHostToDevice));
  CM_HIP(cm::launch_ssim_frames(d_pred, d_gt, N, Cc, H, W, F, (const double *)rng.p, (double *)out.p, nullptr));
  CM_HIP(hipDeviceSynchronize());
  CM_HIP(hipMemcpy(h_out, out.p, cells * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

int cm_energy(int32_t device, const float *d_x, int32_t N, int32_t Cc, int32_t H, int32_t W, int32_t L, float delta_t,
              float delta_l, const float *h_factor, double *h_out) {
  if (!d_x) return fail("cm_energy: d_x is null");
  if (!h_out) return fail("cm_energy: h_out is null");
  if (metric_shape_ok("cm_energy", N, Cc, H, W, L, "L")) return 1;
  if (Cc < 3) return fail("cm_energy: C = %d: the energy reads channels 0-2 (rho, v_x, v_y: guidance.py:25-31), C must be >= 3", Cc);
  if (delta_t == 0.f || delta_l == 0.f) return fail("cm_energy: delta_t = %g and delta_l = %g must be non-zero", delta_t, delta_l);
  const float one[3] = {1.f, 1.f, 1.f};
  DevGuard g(device);
  DevScratch out;
  CM_HIP(out.alloc((size_t)N * sizeof(double)));
  // 1 / delta as the host forms it: a float64 quotient rounded to float32
  CM_HIP(cm::launch_energy(d_x, N, Cc, H, W, L, (float)(1.0 / (double)delta_t), (float)(1.0 / (double)delta_l),
                           h_factor ? h_factor : one, (double *)out.p, nullptr));
  CM_HIP(hipDeviceSynchronize());
  CM_HIP(hipMemcpy(h_out, out.p, (size_t)N * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

int cm_motion_feature_vectors(int32_t device, const float *d_seq, int32_t N, int32_t Cc, int32_t H, int32_t W, int32_t F,
                              int32_t f, int32_t k, double gamma, double *h_mf2, double *h_mf1) {
  if (!d_seq) return fail("cm_motion_feature_vectors: d_seq is null");
  if (!h_mf2) return fail("cm_motion_feature_vectors: h_mf2 is null");
  if (!h_mf1) return fail("cm_motion_feature_vectors: h_mf1 is null");
  long long nvol = 0;
  if (motion_feature_args_ok("cm_motion_feature_vectors", N, Cc, H, W, F, f, k, &nvol)) return 1;
  DevGuard g(device);
  const size_t n2 = (size_t)N * nvol * 256, n1 = (size_t)N * nvol * 16;
  DevScratch mf2, mf1;
  CM_HIP(mf2.alloc(n2 * sizeof(double)));
  CM_HIP(mf1.alloc(n1 * sizeof(double)));
  CM_HIP(cm::launch_motion_features(d_seq, nullptr, N, Cc, H, W, F, f, k, gamma, (double *)mf2.p, (double *)mf1.p, nullptr, nullptr));
  CM_HIP(hipDeviceSynchronize());
  CM_HIP(hipMemcpy(h_mf2, mf2.p, n2 * sizeof(double), hipMemcpyDeviceToHost));
  CM_HIP(hipMemcpy(h_mf1, mf1.p, n1 * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

int cm_motion_feature_tables(int32_t device, const float *d_pred, const float *d_gt, int32_t N, int32_t Cc, int32_t H, int32_t W,
                             int32_t F, int32_t f, int32_t k, double gamma, double *h_out) {
  if (!d_pred) return fail("cm_motion_feature_tables: d_pred is null");
  if (!d_gt) return fail("cm_motion_feature_tables: d_gt is null");
  if (!h_out) return fail("cm_motion_feature_tables: h_out is null");
  long long nvol = 0;
  if (motion_feature_args_ok("cm_motion_feature_tables", N, Cc, H, W, F, f, k, &nvol)) return 1;
  DevGuard g(device);
  DevScratch out;                              // the whole workspace: six numbers per sample
  CM_HIP(out.alloc((size_t)N * 6 * sizeof(double)));
  CM_HIP(cm::launch_motion_features(d_pred, d_gt, N, Cc, H, W, F, f, k, gamma, nullptr, nullptr, (double *)out.p, nullptr));
  CM_HIP(hipDeviceSynchronize());
  CM_HIP(hipMemcpy(h_out, out.p, (size_t)N * 6 * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

}  // extern "C"
