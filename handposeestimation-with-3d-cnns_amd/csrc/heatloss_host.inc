// heatloss_host.inc — the host side of libtsdf_heatloss.so that needs no device: the argument rules of its four entries and
// the coordinate arithmetic its two forward kernels share with them.  Plain C++: tsdf_heatloss.hip includes it (inside its
// anonymous namespace, after include/tsdf_heatloss.h and heatmap_host.inc), and heatloss_host_main.cc includes it into a
// stand-alone program built under the CPU sanitizers (make heatloss-host-asan; tests/test_heatloss_cpu.py runs it).
//   heat_defect_sse, _sse_grad, _soft_argmax, _soft_argmax_grad
//                the first argument rule an entry's arguments break, in the header's order.  The shape rules, the enum and
//                heat_status are heatmap_host.inc's (HeatDefect, heat_defect_shape); bad_res, misaligned and bad_dtype come
//                from the includer as they do there
//   heat_quad    the (slice, row, column) a group of four consecutive elements of a volume starts at
// The gradient kernels' plan and item arithmetic are heatmap_host.inc's heat_plan and heat_item as they are.

// sigma (loss) or beta (soft-argmax): finite and > 0.  A NaN fails the first test, +inf the second.
inline bool heat_bad_positive(float s) { return !(s > 0.f) || !(s <= 3.402823466e38f); }

inline HeatDefect heat_defect_sse(const void *d_pred, int dtype, const float *d_u, const int32_t *d_status, int n, int n_joints,
                                  int R, float sigma, int layout, const double *d_out_sse, const int32_t *d_out_valid) {
  const HeatDefect shape = heat_defect_shape(n, n_joints, R, layout, dtype);
  if (shape != kHeatGood) return shape;
  if (heat_bad_positive(sigma)) return kHeatBadScalar;
  if (!d_pred || !d_u || !d_out_sse) return kHeatNull;
  if (misaligned(d_pred, 15) || misaligned(d_out_sse, 7) || misaligned(d_u, 3) || misaligned(d_status, 3) ||
      misaligned(d_out_valid, 3))
    return kHeatUnaligned;
  if ((int64_t)n * n_joints >= kHeatMaxUnits) return kHeatTooMany;
  return kHeatGood;
}

inline HeatDefect heat_defect_sse_grad(const void *d_pred, int dtype, const float *d_u, const int32_t *d_status,
                                       const float *d_w, int n, int n_joints, int R, float sigma, int layout,
                                       const void *d_out_grad) {
  const HeatDefect shape = heat_defect_shape(n, n_joints, R, layout, dtype);
  if (shape != kHeatGood) return shape;
  if (heat_bad_positive(sigma)) return kHeatBadScalar;
  if (!d_pred || !d_u || !d_w || !d_out_grad) return kHeatNull;
  if (misaligned(d_pred, 15) || misaligned(d_out_grad, 15) || misaligned(d_u, 3) || misaligned(d_status, 3) || misaligned(d_w, 3))
    return kHeatUnaligned;
  if ((int64_t)n * n_joints >= kHeatMaxUnits) return kHeatTooMany;
  return kHeatGood;
}

inline HeatDefect heat_defect_soft_argmax(const void *d_heat, int dtype, int n, int n_joints, int R, float beta, int layout,
                                          const float *d_out_u, const double *d_out_stats) {
  const HeatDefect shape = heat_defect_shape(n, n_joints, R, layout, dtype);
  if (shape != kHeatGood) return shape;
  if (heat_bad_positive(beta)) return kHeatBadScalar;
  if (!d_heat || !d_out_u || !d_out_stats) return kHeatNull;
  if (misaligned(d_heat, 15) || misaligned(d_out_stats, 7) || misaligned(d_out_u, 3)) return kHeatUnaligned;
  if ((int64_t)n * n_joints >= kHeatMaxUnits) return kHeatTooMany;
  return kHeatGood;
}

inline HeatDefect heat_defect_soft_argmax_grad(const void *d_heat, int dtype, const double *d_stats, const float *d_grad_u, int n,
                                               int n_joints, int R, float beta, int layout, const void *d_out_grad) {
  const HeatDefect shape = heat_defect_shape(n, n_joints, R, layout, dtype);
  if (shape != kHeatGood) return shape;
  if (heat_bad_positive(beta)) return kHeatBadScalar;
  if (!d_heat || !d_stats || !d_grad_u || !d_out_grad) return kHeatNull;
  if (misaligned(d_heat, 15) || misaligned(d_out_grad, 15) || misaligned(d_stats, 7) || misaligned(d_grad_u, 3))
    return kHeatUnaligned;
  if ((int64_t)n * n_joints >= kHeatMaxUnits) return kHeatTooMany;
  return kHeatGood;
}

// The forward kernels read a volume in 16-byte pieces numbered in memory order: 4 float32 elements, or 8 of a 2-byte
// dtype — which straddle two rows when R % 8 != 0 (R = 12, 20, 44, ...).  R is a multiple of 4, so a QUAD of four
// consecutive elements starting at a multiple of 4 never does: coordinates are formed per quad, quad q of a volume
// (q < R^3 / 4 <= 2^19) starting at element 4 q.  Two multiply-shifts, as heat_item.
struct HeatQuad {
  int fast, mid, slow;   // the first element's index on the fastest axis; the quad's on the middle and the slowest one
};
TSDF_HEAT_FN HeatQuad heat_quad(unsigned q, int R, unsigned magic_rq, unsigned magic_r) {
  const unsigned RQ = (unsigned)R / 4u;
  const unsigned row = heat_div(q, magic_rq), sl = heat_div(row, magic_r);
  HeatQuad c;
  c.fast = (int)(q - row * RQ) * 4;
  c.mid = (int)(row - sl * (unsigned)R);
  c.slow = (int)sl;
  return c;
}
