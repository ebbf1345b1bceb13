// csrc/mvr_align.hip -- everything that is "an align" (include/mvr_hip.h): the host side of the ICP iteration
// (pcl::IterativeClosestPoint::align) in its four kinds -- plain, with a rejector chain, Generalized ICP,
// target-sharded -- over the search of mvr_ctx.hip, the entry points that run the chain or the GICP optimiser on a caller's
// list, and the sequential drivers.  One host<->device round trip per ICP iteration: the sums come back, the estimator runs
// on the host (GICP: on the device), the new 4x4 goes out as a kernel argument.  The four loops share the bookkeeping around
// an iteration (CurSource, AlignRun); what an iteration DOES stays written out in each loop.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>

#include "mvr_internal.h"

using namespace mvr;      // (the entry points below get their C linkage from their declarations in mvr_hip.h)

// ---- mvr_icp_align of a POSED SCAN (the sequential mode aligns every scan, under its pose so far, against the growing model)
// the current source of an align is an exact copy of a posed scan: give it that scan's pose, grid and grid-ordered
// coordinates, so that the REVERSE searches (matched targets looking for their nearest source point, each with the bound
// its forward match gives) can walk the source's grid instead of the culled kernel's box hierarchy
static bool prepare_source_grid(Ctx *c, const Cloud &posed_src, Cloud &cur, double max_dist)
{
  if (!c->seq_search || c->nn_mode == 0 || !posed_src.pose_known || posed_src.n == 0 || posed_src.n != cur.n) return false;
  if (!(max_dist * max_dist < (double)FLT_MAX)) return false;
  Cloud *src_canon = nullptr;
  for (Cloud &o : c->slots) if (o.set_id == posed_src.set_id && o.canonical && o.n == posed_src.n) { src_canon = &o; break; }
  if (!src_canon) return false;
  if (ensure_grids(c, &src_canon, 1, max_dist + 0.5, c->stream, nullptr) != MVR_OK || !src_canon->grid || src_canon->grid->n != src_canon->n) return false;
  // (the align searches the posed source where it lies: its grid-ordered coordinates may be current already -- the posing launch
  // writes them along when the set has its grid)
  const bool current = &cur == &posed_src && cur.gcoords_valid && cur.grid == src_canon->grid && cur.gsorted;
  cur.pose_known = true; cur.pose_stretch = posed_src.pose_stretch; std::memcpy(cur.pose, posed_src.pose, sizeof cur.pose);
  cur.grid = src_canon->grid;
  if (current) return true;
  cur.gcoords_valid = false;
  Cloud *one = &cur;
  return refresh_grid_coords_batch(c, &one, 1) == MVR_OK && cur.gcoords_valid;
}

// the search of an align's first iteration when the source has its scan's grid (prepare_source_grid): forward = the culled
// kernel over the target's index, every query starting from its seed; reverse = the grid walk over the CURRENT SOURCE's grid
// for the matched targets, compacted by the kernels of the fused pass (no hipCUB).  Leaves keys / slot / rkeys as run_search does.
static int run_search_source_grid(Ctx *c, Cloud &cur, Cloud &tgt, double max_dist, bool reciprocal, bool fma, SearchPlan *plan)
{
  const size_t ns = cur.n, nt = tgt.n;
  const double max2 = max_dist * max_dist;
  const float cap2 = cap_from_max2(max2);
  *plan = SearchPlan();
  if (int rc = ensure(c, c->keys, c->keys_cap, ns)) return rc;
  if (int rc = ensure(c, c->match, c->match_cap, ns)) return rc;
  if (int rc = ensure(c, c->rkeys, c->rkeys_cap, std::max(ns, std::min(ns, nt)))) return rc;
  if (int rc = ensure_index(c, cur)) return rc;
  if (int rc = ensure_index(c, tgt)) return rc;
  plan->qperm = cur.order->perm; plan->tinv = tgt.order->inv;
  if (ns > 0xFFFFFFF0ull || nt > 0xFFFFFFF0ull) return set_error(c, MVR_E_ARG, "cloud too large for 32-bit indices");
  // every query starts from the distance of the point it matched when this scan was last aligned, if it was (Ctx::seq_seed)
  const uint32_t *qb = nullptr;
  if (c->seq_seed) {
    auto it = c->seq_seeds.find(cur.set_id);
    if (it != c->seq_seeds.end() && it->second.d && it->second.n == ns) {
      if (int rc = ensure(c, c->seed_bound, c->seed_bound_cap, ns)) return rc;
      if (int rc = launch_seed_to_bound(c, cur.sorted, ns, tgt.sorted, nt, it->second.d, fma, c->seed_bound)) return rc;
      qb = c->seed_bound;
    }
  }
  // forward: the culled kernel over the target's index (keys are written by exactly one wave per query)
  CullPair fp = make_cull_pair(cur, 0, ns, nullptr, tgt, c->keys);
  fp.qbound = qb;
  if (int rc = launch_nn_cull_batch(c, &fp, 1, cap2, fma)) return rc;
  uint32_t *seed_out = nullptr;
  if (c->seq_seed) {
    if (c->seq_seeds.size() >= 256 && !c->seq_seeds.count(cur.set_id)) {      // (scans that are gone: start over rather than grow without bound)
      MVR_HIP_TRY(c, hipStreamSynchronize(c->stream));
      for (auto &kv : c->seq_seeds) if (kv.second.d) (void)hipFree(kv.second.d);
      c->seq_seeds.clear();
    }
    Ctx::SeedBuf &sb = c->seq_seeds[cur.set_id];
    if (int rc = ensure(c, sb.d, sb.cap, ns)) return rc;
    sb.n = ns;
    seed_out = sb.d;
    // (with reciprocal searches the launch that sets the reverse searches' start bounds walks the same keys: it leaves the seeds)
    if (!reciprocal || nt == 0) { if (int rc = launch_keys_to_seed(c, cur.sorted, ns, c->keys, tgt.order->inv, sb.d)) return rc; }
  }
  if (!reciprocal || nt == 0) return MVR_OK;
  // reverse: the distinct matched targets, each starting from the distance of the source that matched it
  if (int rc = ensure(c, c->bound, c->bound_cap, nt)) return rc;
  if (!c->bwide_count) {
    MVR_MAY_BLOCK(c, "the wide-query counters are not allocated yet");
    MVR_HIP_TRY(c, hipMalloc(&c->bwide_count, 3 * kWideCounters * sizeof(uint32_t)));
    MVR_HIP_TRY(c, hipMemsetAsync(c->bwide_count, 0, 3 * kWideCounters * sizeof(uint32_t), c->stream));
  }
  uint32_t *rev_wide_count = c->bwide_count + kWideCounters - 1;      // (a counter the fused pass does not use; put to zero by the bounds launch)
  if (int rc = launch_seed_bounds(c, c->keys, plan->qperm, 0, ns, max2, plan->tinv, nt, c->bound, seed_out, rev_wide_count)) return rc;
  const size_t nl = std::min(ns, nt), chunks = (nt + 255) / 256;
  if (int rc = ensure(c, c->slot, c->slot_cap, nt)) return rc;
  if (int rc = ensure(c, c->list, c->list_cap, nl)) return rc;
  if (int rc = ensure(c, c->bchunks, c->bchunks_cap, chunks + 8)) return rc;
  if (int rc = ensure(c, c->bwide, c->bwide_cap, nl)) return rc;
  GlueBatch gb;
  gb.max2 = max2; gb.reciprocal = 1; gb.origin[0] = gb.origin[1] = gb.origin[2] = 0.0;
  GluePair &g = gb.p[0];
  g.bound = c->bound; g.list = c->list; g.slot = c->slot; g.chunks = c->bchunks; g.qcount = c->count; g.nt = nt;
  if (int rc = launch_compact_flags_batch(c, gb, 1)) return rc;
  plan->slot = c->slot; plan->count = c->count;
  GridPair rev = make_grid_pair(tgt, 0, nl, cur, c->rkeys);
  rev.qlist = c->list; rev.qcount = c->count; rev.qbound = c->bound;
  rev.wide_list = c->bwide; rev.wide_count = rev_wide_count;
  if (int rc = launch_nn_grid_batch(c, &rev, 1, cap2, fma)) return rc;
  return launch_nn_grid_wide_batch(c, &rev, 1, cap2, fma);
}

// pcl::registration::DefaultConvergenceCriteria::hasConverged, evaluated after every iteration on the
// INCREMENTAL transformation and the mean squared correspondence distance of that iteration
namespace {
struct Criteria {
  double rot_thr, trans_thr, rel_mse, abs_mse = 1e-12, prev_mse = DBL_MAX;
  int max_iterations;
  explicit Criteria(const mvr_icp_params *p)
      : rot_thr(1.0 - p->transformation_epsilon), trans_thr(p->transformation_epsilon), rel_mse(p->euclidean_fitness_eps), max_iterations(p->max_iterations) {}
  bool converged(const float tr[16], double cur_mse, int iters, int *state)
  {
    *state = MVR_CONV_NOT;
    if (iters >= max_iterations) { *state = MVR_CONV_ITERATIONS; return true; }
    const double cos_angle = 0.5 * ((double)tr[0] + (double)tr[5] + (double)tr[10] - 1.0);
    const double t2 = (double)tr[12] * (double)tr[12] + (double)tr[13] * (double)tr[13] + (double)tr[14] * (double)tr[14];
    if (cos_angle >= rot_thr && t2 <= trans_thr) { *state = MVR_CONV_TRANSFORM; return true; }
    if (std::fabs(cur_mse - prev_mse) < abs_mse) { *state = MVR_CONV_ABS_MSE; return true; }
    if (std::fabs(cur_mse - prev_mse) / prev_mse < rel_mse) { *state = MVR_CONV_REL_MSE; return true; }
    prev_mse = cur_mse;
    return false;
  }
};

// The output slot of an align: final * (the ORIGINAL input), alias-safe (registrator.cpp:920).  The one place that keeps the
// slot's bookkeeping, next to finish_dst for the filters; its rule is mvr_cloud_transform_f32's.  To another slot: the source's
// point set (its ordering, not its pose or grid) and the source's segment table -- a slot that was a shard must not number
// the align's points by the table of what it held before.  In place: the slot's points moved by a FLOAT matrix -- they are
// neither the set's upload coordinates nor a known f64 pose of them any more, and a grid built in the old frame must not be
// walked with them; the table stays, as it does for a transform in place.  with_normals: ICP::transformCloud rotates the
// source normals too (the sharded align has none).
int finish_align_out(Ctx *c, int os, int ss, const float fin[16], bool with_normals)
{
  Cloud &o = c->slots[os];
  const Cloud &s = c->slots[ss];
  const size_t ns = s.n;
  if (os != ss) { o.n = 0; if (int rc = cloud_reserve(c, o, ns, false)) return rc; }
  if (int rc = launch_transform_f32(c, s.pts, o.pts, ns, fin)) return rc;
  o.n = ns;
  if (os != ss) { inherit_point_set(o, s); o.segs = s.segs; }
  else o.forget_pose();
  o.stale_coords();
  if (with_normals && s.has_normals && ns) {
    if (int rc = ensure(c, o.nrm, o.nrm_cap, ns)) return rc;
    if (int rc = launch_rotate_normals_f32(c, s.nrm, o.nrm, ns, fin)) return rc;
  }
  o.has_normals = with_normals && s.has_normals;
  return MVR_OK;
}

const float kIdentity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};

// The current source of an align (PCL's input_transformed, App. A.1: guess == identity).  It IS the caller's slot until it
// first moves: the copy PCL makes is only needed by a second iteration, which the reference's settings never reach -- a device
// copy, an index refresh and a grid posing per align that nothing read differently (-25 us of 0.45 ms).  From then on it is the
// scratch cloud, which the later iterations search and move in place.  normals: the source's normals move with it, as
// mvr_cloud_transform_f32 moves a cloud.  sharded: the target-sharded align's two differences -- it copies to the scratch up
// front (start_on_scratch), and a move leaves the pose and grid state alone, which the copy has already forgotten.
struct CurSource {
  Ctx *c;
  const Cloud &orig;
  Cloud &scratch;
  Cloud *cur;
  const size_t n;
  const bool normals, sharded;
  CurSource(Ctx *ctx, int ss, bool with_normals, bool is_sharded = false)
      : c(ctx), orig(ctx->slots[ss]), scratch(ctx->slots[kScratchCur]), cur(&ctx->slots[ss]), n(ctx->slots[ss].n), normals(with_normals), sharded(is_sharded) {}
  Cloud &operator*() const { return *cur; }
  Cloud *operator->() const { return cur; }

  // an exact copy of the source under the source's ordering, numbered locally (a source that was a shard keeps no table)
  int start_on_scratch()
  {
    scratch.n = 0;
    if (int rc = cloud_reserve(c, scratch, n, false)) return rc;
    if (n) { const hipError_t e = hipMemcpyAsync(scratch.pts, orig.pts, n * sizeof(float4), hipMemcpyDeviceToDevice, c->stream); if (e != hipSuccess) return set_error(c, MVR_E_HIP, "copy of the source", e); }
    if (c->nn_mode != 0 && n) { if (int rc = ensure_index(c, *cur)) return rc; }      // sort the source once, share it
    adopt(); scratch.segs.clear();
    return MVR_OK;
  }

  // cur <- tr * cur
  int move(const float tr[16])
  {
    const bool first = cur != &scratch;
    if (first) {
      scratch.n = 0;
      if (int rc = cloud_reserve(c, scratch, n, false)) return rc;
      if (normals) { if (int rc = ensure(c, scratch.nrm, scratch.nrm_cap, n)) return rc; }
    }
    int rc = launch_transform_f32(c, cur->pts, scratch.pts, n, tr);
    if (rc == MVR_OK && normals) rc = launch_rotate_normals_f32(c, cur->nrm, scratch.nrm, n, tr);
    if (first) {
      if (rc != MVR_OK) return rc;
      adopt();
    }
    scratch.stale_coords();
    if (!sharded) { scratch.pose_known = false; scratch.grid.reset(); }
    return rc;
  }

  void done() { scratch.has_normals = false; }      // (where the rejected and the GICP align reset it; the plain align never touches it)

 private:
  void adopt() { scratch.n = n; inherit_point_set(scratch, orig); cur = &scratch; }
};

// The outcome of an align as its loop builds it up, and the one place that hands it to the caller.
struct AlignRun {
  float fin[16], tr[16];          // the product so far, this iteration's increment
  int iters = 0, converged = 0, state = MVR_CONV_NOT, ncorr = 0, status = MVR_OK;
  double cur_mse = 0.0, fwdq = 0.0, evals = 0.0;
  const double t0 = now_ms();
  AlignRun() { std::memcpy(fin, kIdentity, sizeof fin); std::memcpy(tr, kIdentity, sizeof tr); }
  void compose() { mvr_mat4f_mul(tr, fin, fin); ++iters; }
  void fail(int why) { state = MVR_CONV_NO_CORRESPONDENCES; converged = 0; status = why; }      // (PCL's "not enough correspondences" state for every failure)
  // output = final * (*input), from the ORIGINAL input: alias-safe (registrator.cpp:920)
  int finish(Ctx *c, int os, int ss, bool with_normals, float T_out[16], mvr_icp_stats *st) const
  {
    if (os >= 0) { if (int rc = finish_align_out(c, os, ss, fin, with_normals)) return rc; }
    std::memcpy(T_out, fin, sizeof fin);
    if (st) {
      st->iterations = iters; st->converged = converged; st->state = state; st->n_corr = ncorr; st->mse = cur_mse;
      st->evals = evals; st->fwd_queries = fwdq; st->ms = now_ms() - t0;
    }
    return status;
  }
};
}  // namespace

API int mvr_icp_align(mvr_ctx *ctx, int ss, int ts, int os, const mvr_icp_params *p, float T_out[16],
                      mvr_icp_stats *st)
{
  if (!ctx || !slot_ok(ss) || !slot_ok(ts) || (os >= 0 && !slot_ok(os)) || !p || !T_out) return MVR_E_ARG;
  Ctx *c = CTX(ctx);
  MVR_HIP_TRY(c, hipSetDevice(c->device));
  AlignRun run;
  const size_t ns = c->slots[ss].n;
  if (p->point_to_plane && c->slots[ts].n && !c->slots[ts].has_normals)
    return set_error(c, MVR_E_ARG, "point-to-plane needs target normals (mvr_cloud_upload_normals)");
  CurSource cur(c, ss, false);      // (the first iteration searches the source WHERE IT LIES; its scratch copy carries no normals)
  if (c->nn_mode != 0 && ns) { if (int rc = ensure_index(c, c->slots[ss])) return rc; }   // sort the source once, share it
  MVR_HIP_TRY(c, hipMemsetAsync(c->evals + kEvalRegion, 0, kEvalRegion * sizeof(uint64_t), c->stream));   // running totals of the culled kernel
  Criteria crit(p);          // DefaultConvergenceCriteria (App. A.4)
  double evals_total = 0.0;
  Cloud &tgt = c->slots[ts];
  // a posed scan's reverse searches walk its scan's grid -- in the first iteration, while the current source still IS the posed
  // source (later iterations, which the reference's settings never reach, take the culled kernel: the moved source's
  // coordinates are no longer a known pose of its scan)
  const bool rev_grid_ok = ns > 0 && tgt.n > 0 && ts != ss && p->use_reciprocal && tgt.n <= 0xFFFFFFF0ull &&
                           prepare_source_grid(c, c->slots[ss], *cur, p->max_corr_dist);
  // (point-to-point: the iteration's row comes to the host from the last sums launch itself, no copy, no synchronise)
  const bool spin = c->align_spin && !p->point_to_plane && ensure_align_row(c) == MVR_OK;
  do {
    double ev = 0.0;
    SearchPlan plan;
    if (rev_grid_ok && run.iters == 0) { if (int rc = run_search_source_grid(c, *cur, tgt, p->max_corr_dist, p->use_reciprocal != 0, p->fma_dist != 0, &plan)) return rc; }
    else if (int rc = run_search(c, *cur, tgt, 0, ns, p->max_corr_dist, p->use_reciprocal != 0, p->fma_dist != 0, &ev, &plan)) return rc;
    if (int rc = launch_pass1(c, cur->pts, tgt.pts, c->keys, c->rkeys, plan.slot, plan.count, plan.qperm, plan.tinv, 0, ns,
                              p->max_corr_dist * p->max_corr_dist, p->use_reciprocal != 0 && tgt.n > 0, c->match,
                              c->moments)) return rc;
    if (p->point_to_plane) { if (int rc = launch_p2plane(c, cur->pts, tgt.pts, tgt.nrm, c->match, plan.qperm, 0, ns, c->moments + 32)) return rc; }
    else if (int rc = launch_pass2(c, cur->pts, tgt.pts, c->match, plan.qperm, 0, ns, c->moments, (st && c->nn_mode != 0) ? c->evals + kEvalRegion : nullptr,
                               spin ? c->d_align : nullptr, spin ? ++c->align_seq : 0u)) return rc;
    // the search kernels' running evaluation totals ride along with the moments (the statistic needs neither a wait nor a copy
    // of its own: the last sums launch adds the counters up into moments[18]; point-to-plane keeps the copy)
    if (st && c->nn_mode != 0 && p->point_to_plane)
      MVR_HIP_TRY(c, hipMemcpyAsync(c->h_evals, c->evals + kEvalRegion, kEvalRegion * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    if (spin) { if (int rc = spin_moments(c, c->align_seq, 19)) return rc; }
    else if (int rc = read_moments(c, p->point_to_plane ? 64 : 19)) return rc;
    const double *h = c->h_moments;
    if (st && c->nn_mode != 0 && !p->point_to_plane) evals_total = h[18];
    run.fwdq += (double)ns;
    run.evals += (c->nn_mode != 0) ? 0.0 : ev + h[17] * (double)ns;   // forward Ns*Nt + reverse Nt'*Ns (brute force)
    run.ncorr = (int)h[0];
    if (h[0] < 3.0) { run.fail(MVR_E_NOCORR); break; }
    if (p->point_to_plane) {
      if (p2plane_solve(h + 32, h + 32 + 21, run.tr) != MVR_OK) { run.fail(MVR_E_SINGULAR); break; }
    } else umeyama_from_moments(h + 1, h + 4, h + 8, run.tr, nullptr);
    run.cur_mse = h[7];
    run.compose();
    run.converged = crit.converged(run.tr, run.cur_mse, run.iters, &run.state) ? 1 : 0;
    // (the moved source is only needed by another iteration: the output is final * the ORIGINAL input)
    if (!run.converged) { if (int rc = cur.move(run.tr)) return rc; }
  } while (!run.converged);
  if (st && c->nn_mode != 0) {
    run.evals = evals_total;
    if (p->point_to_plane) { run.evals = 0.0; for (int k = 0; k < kEvalShards; ++k) run.evals += (double)c->h_evals[(size_t)k * kEvalStride]; }
  }
  return run.finish(c, os, ss, true, T_out, st);
}

// ---- correspondence rejectors (rules R1-R10 in mvr_hip.h; kernels in mvr_reject.hip)
namespace {
// R10, and R5's normals: everything that is refused before any GPU work
int reject_args(Ctx *c, int ss, int ts, const mvr_rejector *chain, int n_chain, bool *one_to_one)
{
  if (n_chain < 0 || n_chain > MVR_MAX_REJECTORS || (n_chain > 0 && !chain)) return set_error(c, MVR_E_ARG, "rejector chain: n_chain outside 0..MVR_MAX_REJECTORS or a NULL chain");
  const Cloud &s = c->slots[ss], &t = c->slots[ts];
  if (s.n > 0x7FFFFFF0ull || t.n > 0x7FFFFFF0ull) return set_error(c, MVR_E_ARG, "rejector chain: cloud too large");
  if (s.pts_stale || t.pts_stale) return set_error(c, MVR_E_ARG, "rejector chain: a cloud's points are not current (pipelined run)");
  *one_to_one = false;
  for (int k = 0; k < n_chain; ++k) {
    const mvr_rejector &r = chain[k];
    if (r.kind < MVR_REJ_DISTANCE || r.kind > MVR_REJ_SAMPLE_CONSENSUS) return set_error(c, MVR_E_ARG, "rejector chain: unknown kind");
    if (!std::isfinite(r.value)) return set_error(c, MVR_E_ARG, "rejector chain: a value is not finite");
    if (r.kind <= MVR_REJ_TRIMMED && r.value < 0.0) return set_error(c, MVR_E_ARG, "rejector chain: a negative distance, factor or ratio");
    if (r.kind == MVR_REJ_SURFACE_NORMAL && s.n && t.n && !(s.has_normals && t.has_normals))
      return set_error(c, MVR_E_ARG, "the surface-normal rejector needs the normals of both clouds (mvr_cloud_upload_normals)");
    if (r.kind == MVR_REJ_ONE_TO_ONE) *one_to_one = true;
    if (r.kind == MVR_REJ_SAMPLE_CONSENSUS) {      // C12
      if (!(r.value > 0.0)) return set_error(c, MVR_E_ARG, "sample-consensus rejector: the inlier threshold is not > 0");
      if (r.max_iterations > (1u << 24)) return set_error(c, MVR_E_ARG, "sample-consensus rejector: max_iterations above 1 << 24");
    }
  }
  return MVR_OK;
}

inline const uint32_t *reject_words(const Ctx *c) { return reinterpret_cast<const uint32_t *>(c->rej_host + kRejRowDoubles); }

void reject_stages(const Ctx *c, int n_chain, uint32_t *n_found, mvr_rejector_stage *stages, uint32_t *n_corr)
{
  const uint32_t *w = reject_words(c);
  uint32_t live = w[0];
  if (n_found) *n_found = live;
  for (int s = 0; s < n_chain; ++s) {
    const uint32_t *sw = w + kRejHeadWords + s * kRejStageWords;
    if (stages) { stages[s].in = live; stages[s].out = sw[0]; std::memcpy(&stages[s].threshold, &sw[1], 4); }
    live = sw[0];
  }
  if (n_corr) *n_corr = live;
}

// the table after the chain -> the caller's lists (R7), and the stage records
int reject_collect(Ctx *c, size_t ns, int n_chain, int32_t *query, int32_t *match, float *dist2, size_t cap, size_t *m, mvr_rejector_stage *stages)
{
  std::vector<int32_t> hm(ns);
  std::vector<nnkey_t> hk(ns);
  MVR_HIP_TRY(c, hipMemcpyAsync(hm.data(), c->match, ns * 4, hipMemcpyDeviceToHost, c->stream));
  MVR_HIP_TRY(c, hipMemcpyAsync(hk.data(), c->keys, ns * 8, hipMemcpyDeviceToHost, c->stream));
  MVR_HIP_TRY(c, hipMemcpyAsync(c->rej_host, c->rej_row, kRejCopyBytes, hipMemcpyDeviceToHost, c->stream));
  MVR_HIP_TRY(c, hipStreamSynchronize(c->stream));
  size_t k = 0;
  for (size_t i = 0; i < ns; ++i) {
    if (hm[i] < 0) continue;
    if (k < cap) {
      if (query) query[k] = (int32_t)i;
      if (match) match[k] = hm[i];
      if (dist2) { const uint32_t b = (uint32_t)(hk[i] >> 32); std::memcpy(&dist2[k], &b, 4); }
    }
    ++k;
  }
  uint32_t n_corr = 0;
  reject_stages(c, n_chain, nullptr, stages, &n_corr);
  if ((size_t)n_corr != k) return set_error(c, MVR_E_HIP, "rejector chain: the stage counts and the table disagree");
  *m = k;
  return MVR_OK;
}
}  // namespace

API int mvr_correspondences_rejected(mvr_ctx *ctx, int ss, int ts, double max_dist, int reciprocal, int fma, const mvr_rejector *chain,
                                     int n_chain, int32_t *query, int32_t *match, float *dist2, size_t cap, size_t *m,
                                     mvr_rejector_stage *stages)
{
  if (!ctx || !slot_ok(ss) || !slot_ok(ts) || !m) return MVR_E_ARG;
  Ctx *c = CTX(ctx);
  bool oto = false;
  if (int rc = reject_args(c, ss, ts, chain, n_chain, &oto)) return rc;
  MVR_HIP_TRY(c, hipSetDevice(c->device));
  *m = 0;
  if (stages) std::memset(stages, 0, sizeof(mvr_rejector_stage) * (size_t)n_chain);
  const size_t ns = c->slots[ss].n, nt = c->slots[ts].n;
  if (ns == 0 || nt == 0) return MVR_OK;
  if (int rc = ensure_reject_state(c, nt, oto)) return rc;
  SearchPlan plan;
  if (int rc = pair_common(c, ss, ts, max_dist, reciprocal, fma, 0, ns, nullptr, &plan)) return rc;
  if (int rc = launch_reject_chain(c, chain, n_chain, c->keys, c->match, ns, nt, c->slots[ss].nrm, c->slots[ts].nrm, c->moments, 0u,
                                   c->slots[ss].pts, c->slots[ts].pts, fma != 0)) return rc;
  return reject_collect(c, ns, n_chain, query, match, dist2, cap, m, stages);
}

namespace {
// R8: a caller's correspondence list, checked on the host while it is laid out as the search would have left it -- hm: match[]
// by source index (-1: no entry); hk, if wanted: the keys (d2 bits << 32 | match), which needs dist2.  prefix: who refuses
// ("rejector list", "GICP list"; the rejector's clouds have passed the first two checks in reject_args already, as "rejector
// chain: ...").  no_normals: the refusal of a non-empty list between clouds without normals (GICP), or null.
int layout_list(Ctx *c, const char *prefix, const Cloud &s, const Cloud &t, const int32_t *query, const int32_t *match, const float *dist2,
                size_t count, std::vector<int32_t> &hm, std::vector<nnkey_t> *hk, const char *no_normals)
{
  const auto refuse = [&](const char *what) { return set_error(c, MVR_E_ARG, (std::string(prefix) + what).c_str()); };
  if (s.n > 0x7FFFFFF0ull || t.n > 0x7FFFFFF0ull) return refuse(": cloud too large");
  if (s.pts_stale || t.pts_stale) return refuse(": a cloud's points are not current (pipelined run)");
  if (count > s.n) return refuse(": more entries than source points (query indices must be distinct)");
  if (no_normals && count && !(s.has_normals && t.has_normals)) return set_error(c, MVR_E_ARG, no_normals);
  hm.assign(s.n, -1);
  if (hk) *hk = std::vector<nnkey_t>(s.n, kKeyInit);
  for (size_t k = 0; k < count; ++k) {
    if (query[k] < 0 || (size_t)query[k] >= s.n || match[k] < 0 || (size_t)match[k] >= t.n) return refuse(": index out of range");
    if (hm[query[k]] >= 0) return refuse(": a query index appears twice");
    hm[query[k]] = match[k];
    if (!hk) continue;
    if (!(dist2[k] >= 0.0f)) return refuse(": a squared distance is negative or NaN");
    uint32_t b; std::memcpy(&b, &dist2[k], 4);
    if (b == 0x80000000u) b = 0u;                      // (-0 compares >= 0: taken as +0, so that the patterns order as the values)
    (*hk)[query[k]] = ((nnkey_t)b << 32) | (nnkey_t)(uint32_t)match[k];
  }
  return MVR_OK;
}

// R8: the chain on the caller's list (sac_trace: what a SAMPLE_CONSENSUS stage records, for the dedicated entry)
int reject_list(mvr_ctx *ctx, int ss, int ts, const int32_t *query, const int32_t *match, const float *dist2, size_t count,
                const mvr_rejector *chain, int n_chain, int32_t *q_out, int32_t *m_out, float *d_out, size_t cap, size_t *m,
                mvr_rejector_stage *stages, mvr_rej_sac_trace *sac_trace, size_t sac_trace_cap)
{
  if (!ctx || !slot_ok(ss) || !slot_ok(ts) || !m || (count && (!query || !match || !dist2))) return MVR_E_ARG;
  Ctx *c = CTX(ctx);
  bool oto = false;
  if (int rc = reject_args(c, ss, ts, chain, n_chain, &oto)) return rc;
  const size_t ns = c->slots[ss].n, nt = c->slots[ts].n;
  std::vector<int32_t> hm;
  std::vector<nnkey_t> hk;
  if (int rc = layout_list(c, "rejector list", c->slots[ss], c->slots[ts], query, match, dist2, count, hm, &hk, nullptr)) return rc;
  MVR_HIP_TRY(c, hipSetDevice(c->device));
  *m = 0;
  if (stages) std::memset(stages, 0, sizeof(mvr_rejector_stage) * (size_t)n_chain);
  if (ns == 0 || nt == 0 || count == 0) return MVR_OK;
  if (int rc = ensure_reject_state(c, nt, oto)) return rc;
  if (int rc = ensure(c, c->keys, c->keys_cap, ns)) return rc;
  if (int rc = ensure(c, c->match, c->match_cap, ns)) return rc;
  MVR_HIP_TRY(c, hipMemcpyAsync(c->match, hm.data(), ns * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
  MVR_HIP_TRY(c, hipMemcpyAsync(c->keys, hk.data(), ns * sizeof(nnkey_t), hipMemcpyHostToDevice, c->stream));
  MVR_HIP_TRY(c, hipStreamSynchronize(c->stream));     // (pageable sources: the vectors are reused below)
  if (int rc = launch_reject_chain(c, chain, n_chain, c->keys, c->match, ns, nt, c->slots[ss].nrm, c->slots[ts].nrm, nullptr, (uint32_t)count,
                                   c->slots[ss].pts, c->slots[ts].pts, false, sac_trace, sac_trace_cap)) return rc;
  return reject_collect(c, ns, n_chain, q_out, m_out, d_out, cap, m, stages);
}
}  // namespace

API int mvr_reject_correspondences(mvr_ctx *ctx, int ss, int ts, const int32_t *query, const int32_t *match, const float *dist2, size_t count,
                                   const mvr_rejector *chain, int n_chain, int32_t *q_out, int32_t *m_out, float *d_out, size_t cap,
                                   size_t *m, mvr_rejector_stage *stages)
{
  return reject_list(ctx, ss, ts, query, match, dist2, count, chain, n_chain, q_out, m_out, d_out, cap, m, stages, nullptr, 0);
}

// the sample-consensus rejector on the caller's list, with its full evidence (rules C1-C12)
API int mvr_reject_sample_consensus(mvr_ctx *ctx, int ss, int ts, const int32_t *query, const int32_t *match, const float *dist2, size_t count,
                                    const mvr_rejector *r, mvr_rej_sac_result *result, int32_t *q_out, int32_t *m_out, float *d_out, size_t cap,
                                    size_t *m, mvr_rej_sac_trace *trace, size_t trace_cap)
{
  if (!ctx || !r || !result || r->kind != MVR_REJ_SAMPLE_CONSENSUS) return MVR_E_ARG;
  Ctx *c = CTX(ctx);
  const bool had = c->last_sac_set;
  c->last_sac_set = false;
  const int rc = reject_list(ctx, ss, ts, query, match, dist2, count, r, 1, q_out, m_out, d_out, cap, m, nullptr, trace, trace_cap);
  const bool ran = c->last_sac_set;
  c->last_sac_set = had || ran;
  if (rc != MVR_OK) return rc;
  if (ran) *result = c->last_sac;
  else reject_sac_identity(result);      // an empty cloud or list: no stage ran
  return MVR_OK;
}

API int mvr_ctx_last_sample_consensus(mvr_ctx *ctx, mvr_rej_sac_result *result)
{
  if (!ctx || !result) return MVR_E_ARG;
  Ctx *c = CTX(ctx);
  if (!c->last_sac_set) return set_error(c, MVR_E_ARG, "no sample-consensus rejector has run on this context");
  *result = c->last_sac;
  return MVR_OK;
}

// PCL's computeTransformation with rejectors (R9).  The loop of mvr_icp_align with the chain between the search and the sums;
// the sums are the raw second moments over the rewritten match[] (and the point-to-plane normal equations), which come to the
// host in ONE copy together with the stages' counts and thresholds.
API int mvr_icp_align_rejected(mvr_ctx *ctx, int ss, int ts, int os, const mvr_icp_params *p, const mvr_rejector *chain, int n_chain,
                               float T_out[16], mvr_icp_stats *st, mvr_icp_iter_trace *trace, int trace_cap)
{
  if (!ctx || !slot_ok(ss) || !slot_ok(ts) || (os >= 0 && !slot_ok(os)) || !p || !T_out || (trace && trace_cap < 0)) return MVR_E_ARG;
  Ctx *c = CTX(ctx);
  bool oto = false;
  if (int rc = reject_args(c, ss, ts, chain, n_chain, &oto)) return rc;
  Cloud &tgt = c->slots[ts];
  if (p->point_to_plane && tgt.n && !tgt.has_normals)
    return set_error(c, MVR_E_ARG, "point-to-plane needs target normals (mvr_cloud_upload_normals)");
  MVR_HIP_TRY(c, hipSetDevice(c->device));
  AlignRun run;
  const size_t ns = c->slots[ss].n, nt = tgt.n;
  CurSource cur(c, ss, c->slots[ss].has_normals && ns);      // (the source's normals move with it if it has any)
  Criteria crit(p);
  double origin[3] = {0.0, 0.0, 0.0};
  if (ns == 0 || nt == 0) run.fail(MVR_E_NOCORR);
  else {
    if (int rc = ensure_reject_state(c, nt, oto)) return rc;
    if (c->nn_mode != 0) { if (int rc = ensure_index(c, c->slots[ss])) return rc; }
  }
  while (run.status == MVR_OK && !run.converged) {
    SearchPlan plan;
    if (int rc = run_search(c, *cur, tgt, 0, ns, p->max_corr_dist, p->use_reciprocal != 0, p->fma_dist != 0, nullptr, &plan)) return rc;
    if (int rc = launch_pass1(c, cur->pts, tgt.pts, c->keys, c->rkeys, plan.slot, plan.count, plan.qperm, plan.tinv, 0, ns,
                              p->max_corr_dist * p->max_corr_dist, p->use_reciprocal != 0, c->match, c->moments)) return rc;
    if (int rc = launch_reject_chain(c, chain, n_chain, c->keys, c->match, ns, nt, cur->nrm, tgt.nrm, c->moments, 0u, cur->pts, tgt.pts,
                                     p->fma_dist != 0)) return rc;
    if (int rc = launch_moments2(c, cur->pts, tgt.pts, c->match, c->keys, plan.qperm, 0, ns, origin, c->rej_row)) return rc;
    if (p->point_to_plane) { if (int rc = launch_p2plane(c, cur->pts, tgt.pts, tgt.nrm, c->match, plan.qperm, 0, ns, c->rej_row + 32)) return rc; }
    MVR_HIP_TRY(c, hipMemcpyAsync(c->rej_host, c->rej_row, kRejCopyBytes, hipMemcpyDeviceToHost, c->stream));      // the iteration's one round trip
    MVR_HIP_TRY(c, hipStreamSynchronize(c->stream));
    const double *h = c->rej_host;
    mvr_icp_iter_trace *tk = (trace && run.iters < trace_cap) ? &trace[run.iters] : nullptr;
    uint32_t n_found = 0, n_live = 0;
    if (tk) std::memset(tk, 0, sizeof *tk);
    reject_stages(c, n_chain, &n_found, tk ? tk->stages : nullptr, &n_live);
    if ((double)n_live != h[0]) return set_error(c, MVR_E_HIP, "mvr_icp_align_rejected: the stage counts and the sums disagree");
    run.fwdq += (double)ns;
    run.ncorr = (int)n_live;
    if (tk) { tk->n_found = n_found; tk->n_corr = n_live; std::memcpy(tk->tr, kIdentity, sizeof kIdentity); }
    if (n_live < 3u) { run.fail(MVR_E_NOCORR); break; }
    mvr_pair_moments2_t m2;
    static_assert(sizeof m2 == 32 * sizeof(double), "moments2 layout");
    std::memcpy(&m2, h, sizeof m2);
    mvr_pair_moments_t mom;
    if (int rc = mvr_moments_from_moments2(&m2, &mom)) return set_error(c, rc, "moments of the rejected align");
    if (p->point_to_plane) {
      if (p2plane_solve(h + 32, h + 32 + 21, run.tr) != MVR_OK) { run.fail(MVR_E_SINGULAR); break; }
    } else umeyama_from_moments(mom.mean_src, mom.mean_tgt, mom.sigma, run.tr, nullptr);
    run.cur_mse = h[31] / h[0];                          // mean of the survivors' (f32) squared distances, summed in f64
    for (int k = 0; k < 3; ++k) origin[k] = mom.mean_tgt[k];      // the next iteration's sums are taken about this one's target mean
    if (tk) { tk->mse = run.cur_mse; std::memcpy(tk->tr, run.tr, sizeof run.tr); }
    run.compose();
    run.converged = crit.converged(run.tr, run.cur_mse, run.iters, &run.state) ? 1 : 0;
    if (!run.converged) { if (int rc = cur.move(run.tr)) return rc; }
  }
  cur.done();
  return run.finish(c, os, ss, true, T_out, st);
}

// ---- Generalized ICP (rules G1-G10 in mvr_hip.h; kernels and the optimiser's driver in mvr_gicp.hip)
API void mvr_gicp_default_params(mvr_gicp_params *p)
{
  if (!p) return;
  p->max_corr_dist = 5.0; p->use_reciprocal = 0; p->fma_dist = 0; p->max_iterations = 200; p->max_inner_iterations = 20;
  p->transformation_epsilon = 5e-4; p->rotation_epsilon = 2e-3; p->gicp_epsilon = 1e-3; p->inner_rot_tol = 1e-6;
  p->inner_trans_tol = 1e-5; p->inner_chunk = 4;
}

namespace {
const char kGicpNeedsNormals[] = "GICP needs the normals of both clouds (mvr_cloud_upload_normals / mvr_cloud_estimate_normals)";

// G10's own refusals and G1's normals
int gicp_args(Ctx *c, int ss, int ts, const mvr_gicp_params *p)
{
  const auto pos = [](double v) { return std::isfinite(v) && v > 0.0; };
  if (!(p->gicp_epsilon > 0.0 && p->gicp_epsilon <= 1.0)) return set_error(c, MVR_E_ARG, "GICP: gicp_epsilon outside (0, 1]");
  if (!pos(p->transformation_epsilon) || !pos(p->rotation_epsilon) || !pos(p->inner_rot_tol) || !pos(p->inner_trans_tol))
    return set_error(c, MVR_E_ARG, "GICP: an epsilon or a tolerance is not positive and finite");
  if (p->max_inner_iterations < 1) return set_error(c, MVR_E_ARG, "GICP: max_inner_iterations < 1");
  const Cloud &s = c->slots[ss], &t = c->slots[ts];
  if (s.n && t.n && !(s.has_normals && t.has_normals)) return set_error(c, MVR_E_ARG, kGicpNeedsNormals);
  return MVR_OK;
}

// the caller's list, validated as in R8 and laid out as the search would have left it: match[] by source index
int gicp_list(Ctx *c, int ss, int ts, const int32_t *query, const int32_t *match, size_t count)
{
  const Cloud &s = c->slots[ss], &t = c->slots[ts];
  std::vector<int32_t> hm;
  if (int rc = layout_list(c, "GICP list", s, t, query, match, nullptr, count, hm, nullptr, kGicpNeedsNormals)) return rc;
  if (count == 0) return MVR_OK;
  MVR_HIP_TRY(c, hipSetDevice(c->device));
  if (int rc = ensure_gicp_state(c)) return rc;
  if (int rc = ensure(c, c->match, c->match_cap, s.n)) return rc;
  MVR_HIP_TRY(c, hipMemcpyAsync(c->match, hm.data(), s.n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
  MVR_HIP_TRY(c, hipStreamSynchronize(c->stream));     // hm goes out of scope
  return MVR_OK;
}

inline const uint32_t *gicp_host_words(const Ctx *c) { return reinterpret_cast<const uint32_t *>(c->gicp_host + kGicpWordsAt); }

// R row-major + t of the state block -> 4x4 column-major
void gicp_mat(const double *x, double *T)
{
  for (int k = 0; k < 16; ++k) T[k] = 0.0;
  for (int r = 0; r < 3; ++r) { for (int k = 0; k < 3; ++k) T[r + 4 * k] = x[3 * r + k]; T[12 + r] = x[9 + r]; }
  T[15] = 1.0;
}

int gicp_ride(Ctx *c)      // the chain's words and the sum of the survivors' d2 come with the optimiser's first round trip
{
  MVR_HIP_TRY(c, hipMemcpyAsync(c->rej_host, c->rej_row, kRejCopyBytes, hipMemcpyDeviceToHost, c->stream));
  return MVR_OK;
}
}  // namespace

API int mvr_gicp_sums(mvr_ctx *ctx, int ss, int ts, const int32_t *query, const int32_t *match, size_t count, const double X[16],
                      double eps, double out[29])
{
  if (!ctx || !slot_ok(ss) || !slot_ok(ts) || !X || !out || (count && (!query || !match))) return MVR_E_ARG;
  Ctx *c = CTX(ctx);
  if (!(eps > 0.0 && eps <= 1.0)) return set_error(c, MVR_E_ARG, "GICP: gicp_epsilon outside (0, 1]");
  for (int k = 0; k < 16; ++k) if (!std::isfinite(X[k])) return set_error(c, MVR_E_ARG, "GICP: X is not finite");
  if (int rc = gicp_list(c, ss, ts, query, match, count)) return rc;
  for (int k = 0; k < 29; ++k) out[k] = 0.0;
  if (count == 0) return MVR_OK;
  const Cloud &s = c->slots[ss], &t = c->slots[ts];
  if (int rc = launch_gicp_init(c, X)) return rc;
  if (int rc = launch_gicp_pairs(c, s.pts, s.nrm, t.pts, t.nrm, c->match, nullptr, 0, s.n, nullptr, eps, true, 1)) return rc;
  if (int rc = read_gicp_state(c)) return rc;
  std::memcpy(out, c->gicp_host + kGicpSums, 29 * sizeof(double));
  return MVR_OK;
}

API int mvr_gicp_solve(mvr_ctx *ctx, int ss, int ts, const int32_t *query, const int32_t *match, size_t count, const mvr_gicp_params *p,
                       double X_out[16], mvr_gicp_info *info)
{
  if (!ctx || !slot_ok(ss) || !slot_ok(ts) || !p || !X_out || (count && (!query || !match))) return MVR_E_ARG;
  Ctx *c = CTX(ctx);
  if (int rc = gicp_args(c, ss, ts, p)) return rc;
  if (int rc = gicp_list(c, ss, ts, query, match, count)) return rc;
  const double I[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
  gicp_mat(I, X_out);
  if (info) std::memset(info, 0, sizeof *info);
  if (count < 3) return set_error(c, MVR_E_NOCORR, "GICP: fewer than 3 correspondences");
  const Cloud &s = c->slots[ss], &t = c->slots[ts];
  if (int rc = gicp_optimise(c, s.pts, s.nrm, t.pts, t.nrm, c->match, nullptr, 0, s.n, p, nullptr)) return rc;
  const double *h = c->gicp_host;
  const uint32_t *w = gicp_host_words(c);
  gicp_mat(h + kGicpX, X_out);
  if (info) { info->evaluations = w[kGicpEvals]; info->accepted = w[kGicpAccepted]; info->lambda = h[kGicpLambda]; info->f0 = h[kGicpF0]; info->f1 = h[kGicpF1]; }
  const int status = (int)w[kGicpStatus];
  if (status != MVR_OK) return set_error(c, status, "GICP: the inner optimisation stopped (a pivot of the damped system is not positive, or f at X = I is not finite)");
  return MVR_OK;
}

// PCL's GeneralizedIterativeClosestPoint::computeTransformation (G2, G8): the loop of mvr_icp_align_rejected with the device's
// Levenberg-Marquardt in the estimator's place.  Search, chain, the sum of the survivors' d2 and the first chunk of the
// optimiser are queued behind each other; the first round trip of the optimiser brings the chain's words along.
API int mvr_icp_align_gicp(mvr_ctx *ctx, int ss, int ts, int os, const mvr_gicp_params *p, const mvr_rejector *chain, int n_chain,
                           float T_out[16], mvr_icp_stats *st, mvr_gicp_iter_trace *trace, int trace_cap)
{
  if (!ctx || !slot_ok(ss) || !slot_ok(ts) || (os >= 0 && !slot_ok(os)) || !p || !T_out || (trace && trace_cap < 0)) return MVR_E_ARG;
  Ctx *c = CTX(ctx);
  bool oto = false;
  if (int rc = reject_args(c, ss, ts, chain, n_chain, &oto)) return rc;
  if (int rc = gicp_args(c, ss, ts, p)) return rc;
  Cloud &tgt = c->slots[ts];
  MVR_HIP_TRY(c, hipSetDevice(c->device));
  AlignRun run;
  const size_t ns = c->slots[ss].n, nt = tgt.n;
  CurSource cur(c, ss, true);      // (G1: a source that is searched has its normals, and they move with it)
  const double origin[3] = {0.0, 0.0, 0.0};
  if (ns == 0 || nt == 0) run.fail(MVR_E_NOCORR);
  else {
    if (int rc = ensure_reject_state(c, nt, oto)) return rc;
    if (int rc = ensure_gicp_state(c)) return rc;
    if (c->nn_mode != 0) { if (int rc = ensure_index(c, c->slots[ss])) return rc; }
  }
  while (run.status == MVR_OK && !run.converged) {
    SearchPlan plan;
    if (int rc = run_search(c, *cur, tgt, 0, ns, p->max_corr_dist, p->use_reciprocal != 0, p->fma_dist != 0, nullptr, &plan)) return rc;
    if (int rc = launch_pass1(c, cur->pts, tgt.pts, c->keys, c->rkeys, plan.slot, plan.count, plan.qperm, plan.tinv, 0, ns,
                              p->max_corr_dist * p->max_corr_dist, p->use_reciprocal != 0, c->match, c->moments)) return rc;
    if (int rc = launch_reject_chain(c, chain, n_chain, c->keys, c->match, ns, nt, cur->nrm, tgt.nrm, c->moments, 0u, cur->pts, tgt.pts,
                                     p->fma_dist != 0)) return rc;
    if (int rc = launch_moments2(c, cur->pts, tgt.pts, c->match, c->keys, plan.qperm, 0, ns, origin, c->rej_row)) return rc;      // (count and the sum of d2)
    if (int rc = gicp_optimise(c, cur->pts, cur->nrm, tgt.pts, tgt.nrm, c->match, plan.qperm, 0, ns, p, gicp_ride)) return rc;
    const double *h = c->rej_host, *g = c->gicp_host;
    const uint32_t *w = gicp_host_words(c);
    mvr_gicp_iter_trace *tk = (trace && run.iters < trace_cap) ? &trace[run.iters] : nullptr;
    uint32_t n_found = 0, n_live = 0;
    if (tk) std::memset(tk, 0, sizeof *tk);
    reject_stages(c, n_chain, &n_found, tk ? tk->stages : nullptr, &n_live);
    if ((double)n_live != h[0] || (double)n_live != g[kGicpSums + 27]) return set_error(c, MVR_E_HIP, "mvr_icp_align_gicp: the stage counts and the sums disagree");
    run.fwdq += (double)ns;
    run.ncorr = (int)n_live;
    if (tk) { tk->n_found = n_found; tk->n_corr = n_live; std::memcpy(tk->tr, kIdentity, sizeof kIdentity); }
    if (n_live < 3u) { run.fail(MVR_E_NOCORR); break; }
    run.cur_mse = h[31] / h[0];                          // mean of the survivors' (f32) squared distances, summed in f64
    if (tk) {
      tk->mse = run.cur_mse; tk->f0 = g[kGicpF0]; tk->f1 = g[kGicpF1]; tk->inner_evals = w[kGicpEvals]; tk->inner_accepted = w[kGicpAccepted];
      tk->lambda = g[kGicpLambda];
    }
    if ((int)w[kGicpStatus] != MVR_OK) { run.fail((int)w[kGicpStatus]); break; }
    double Xd[16];
    gicp_mat(g + kGicpX, Xd);
    for (int k = 0; k < 16; ++k) run.tr[k] = (float)Xd[k];                 // G8: X rounded to f32
    if (tk) std::memcpy(tk->tr, run.tr, sizeof run.tr);
    float before[16];
    std::memcpy(before, run.fin, sizeof before);
    run.compose();
    double delta = 0.0;      // G8: the largest change of an entry of the product, in units of its epsilon
    for (int k = 0; k < 3; ++k) {
      for (int r = 0; r < 3; ++r) delta = std::max(delta, std::fabs((double)run.fin[r + 4 * k] - (double)before[r + 4 * k]) / p->rotation_epsilon);
      delta = std::max(delta, std::fabs((double)run.fin[12 + k] - (double)before[12 + k]) / p->transformation_epsilon);
    }
    if (delta < 1.0) { run.state = MVR_CONV_TRANSFORM; run.converged = 1; }
    else if (run.iters >= p->max_iterations) { run.state = MVR_CONV_ITERATIONS; run.converged = 1; }
    if (!run.converged) { if (int rc = cur.move(run.tr)) return rc; }
  }
  cur.done();
  if (run.status == MVR_E_SINGULAR) (void)set_error(c, MVR_E_SINGULAR, "mvr_icp_align_gicp: a pivot of the damped system is not positive");
  return run.finish(c, os, ss, true, T_out, st);
}

// ---- Normal Distributions Transform (rules N1-N12 in mvr_hip.h; kernels in mvr_ndt.hip, the host's matrices and the 6x6
// eigen-decomposition in host_math.cpp).  An evaluation is two launches and a 232-byte read-back; the Newton loop with its
// backtracking line search runs here.
API void mvr_ndt_default_params(mvr_ndt_params *p)
{
  if (!p) return;
  p->resolution = 1.0; p->step_size = 0.1; p->outlier_ratio = 0.55; p->transformation_epsilon = 0.1; p->min_covar_eigvalue_mult = 0.01;
  p->origin[0] = p->origin[1] = p->origin[2] = 0.0;
  p->max_iterations = 35; p->max_line_evals = 10; p->min_points_per_voxel = 6;
}

namespace {
// N11's parameter checks, with the refusal in the context's error text
int ndt_check(Ctx *c, const mvr_ndt_params *p, const double *guess, double d123[3])
{
  const char *why = "";
  const int rc = ndt_args(p, guess, d123, &why);
  return rc == MVR_OK ? MVR_OK : set_error(c, rc, why);
}
}  // namespace

API int mvr_ndt_constants(const mvr_ndt_params *p, const double *guess, double d123[3])
{
  if (!p || !d123) return MVR_E_ARG;
  double d[3];
  if (int rc = ndt_args(p, guess, d, nullptr)) return rc;
  std::memcpy(d123, d, sizeof d);
  return MVR_OK;
}

API int mvr_ndt_direction(const double sums[29], double delta[6])
{
  if (!sums || !delta) return MVR_E_ARG;
  return ndt_direction(sums, delta);
}

API int mvr_ndt_cells(mvr_ctx *ctx, int ts, const mvr_ndt_params *p, size_t cap, uint64_t *key, uint32_t *count, double *mean, double *icov,
                      size_t *n)
{
  if (!ctx || !slot_ok(ts) || !p || !n) return MVR_E_ARG;
  Ctx *c = CTX(ctx);
  double d[3];
  if (int rc = ndt_check(c, p, nullptr, d)) return rc;
  MVR_HIP_TRY(c, hipSetDevice(c->device));
  NdtCells cells;
  if (int rc = ndt_build_cells(c, c->slots[ts], p, &cells)) return rc;
  *n = cells.n;
  const size_t m = std::min<size_t>(cap, cells.n);
  if (m) {
    static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "cell keys");
    if (key) MVR_HIP_TRY(c, hipMemcpyAsync(key, cells.key, m * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    if (count) MVR_HIP_TRY(c, hipMemcpyAsync(count, cells.count, m * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if (mean) MVR_HIP_TRY(c, hipMemcpyAsync(mean, cells.mean, 3 * m * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (icov) MVR_HIP_TRY(c, hipMemcpyAsync(icov, cells.icov, 6 * m * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    MVR_HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  return MVR_OK;
}

API int mvr_ndt_sums(mvr_ctx *ctx, int ss, int ts, const mvr_ndt_params *p, const double *guess, const double x[6], double out[29])
{
  if (!ctx || !slot_ok(ss) || !slot_ok(ts) || !p || !x || !out) return MVR_E_ARG;
  Ctx *c = CTX(ctx);
  double d[3];
  if (int rc = ndt_check(c, p, guess, d)) return rc;
  for (int k = 0; k < 6; ++k) if (!std::isfinite(x[k])) return set_error(c, MVR_E_ARG, "NDT: the pose is not finite");
  MVR_HIP_TRY(c, hipSetDevice(c->device));
  NdtCells cells;
  if (int rc = ndt_build_cells(c, c->slots[ts], p, &cells)) return rc;
  NdtPose P;
  ndt_pose(p, d, guess, x, &P);
  return ndt_eval(c, c->slots[ss], cells, P, out);
}

API int mvr_ndt_align(mvr_ctx *ctx, int ss, int ts, int os, const mvr_ndt_params *p, const double *guess, float T_out[16], double X_out[16],
                      mvr_ndt_stats *st, mvr_ndt_iter_trace *trace, int trace_cap)
{
  if (!ctx || !slot_ok(ss) || !slot_ok(ts) || (os >= 0 && (!slot_ok(os) || os == ss || os == ts)) || !p || !T_out || (trace && trace_cap < 0))
    return MVR_E_ARG;
  Ctx *c = CTX(ctx);
  double d[3];
  if (int rc = ndt_check(c, p, guess, d)) return rc;
  MVR_HIP_TRY(c, hipSetDevice(c->device));
  const double t0 = now_ms();
  const Cloud &src = c->slots[ss];
  NdtCells cells;
  if (int rc = ndt_build_cells(c, c->slots[ts], p, &cells)) return rc;
  // N7-N9: the loop is host_math.cpp's ndt_newton; an evaluation is the pose's matrices, two launches and a read-back
  struct Eval { Ctx *c; const Cloud *src; const NdtCells *cells; const mvr_ndt_params *p; const double *d, *guess; } ev = {c, &src, &cells, p, d, guess};
  const mvr_ndt_eval_fn eval = [](void *user, const double xp[6], double sums[29]) -> int {
    const Eval *e = static_cast<const Eval *>(user);
    NdtPose Q;
    ndt_pose(e->p, e->d, e->guess, xp, &Q);
    return ndt_eval(e->c, *e->src, *e->cells, Q, sums);
  };
  double x[6], cur[29];
  mvr_ndt_stats run = {};
  const int status = ndt_newton(p, eval, &ev, x, cur, &run, trace, trace_cap);
  if (status != MVR_OK && status != MVR_E_NOCORR) return status;
  NdtPose P;
  // N10
  ndt_pose(p, d, guess, x, &P);
  double X[16];
  float T[16];
  ndt_matrix(P, X);
  for (int k = 0; k < 16; ++k) T[k] = (float)X[k];
  if (os >= 0) { if (int rc = finish_align_out(c, os, ss, T, false)) return rc; }
  std::memcpy(T_out, T, sizeof T);
  if (X_out) std::memcpy(X_out, X, sizeof X);
  if (st) {
    *st = run;
    st->n_cells = cells.n; st->ms = now_ms() - t0;
  }
  return status;
}

// ---- sequential mode with the growing target SHARDED by points over the ranks (registrator.cpp:563-577 is
// loop-carried and does not shard by pair).  One IterativeClosestPoint::align of the full source (every rank holds it)
// against the distributed target, as one native loop per rank:
//   forward NN in the rank's shard -> Ns signed keys (d2 bits << 32 | GLOBAL target index)
//   ncclAllReduce(ncclInt64, ncclMin) of the keys on the context's stream     (ties -> lowest global index: the single-GPU rule)
//   reciprocal check + raw second moments of the matches whose target the rank OWNS
//   ncclAllReduce(ncclDouble, ncclSum) of the 32 sums (+ the iteration's failure count)
//   one D2H of 40 doubles, Umeyama on the host, convergence criteria, transform of the current source
// A rank whose local work fails still joins both collectives of the iteration, with neutral contributions and a raised
// failure count: every rank then leaves the loop in the same iteration with an error instead of one rank leaving its
// peers inside a collective.  Without a communicator the context is a world of one and the collectives are no-ops.
API int mvr_seq_align_sharded(mvr_ctx *ctx, int ss, int ts, int os, const mvr_icp_params *p, const double origin[3], float T_out[16],
                              mvr_icp_stats *st)
{
  if (!ctx || !slot_ok(ss) || !slot_ok(ts) || (os >= 0 && !slot_ok(os)) || !p || !origin || !T_out || ss == ts || os == ts) return MVR_E_ARG;
  Ctx *c = CTX(ctx);
  MVR_HIP_TRY(c, hipSetDevice(c->device));
  if (p->point_to_plane) return set_error(c, MVR_E_ARG, "the sharded align is point-to-point (the reference's estimator)");
  if (c->comm_broken) return set_error(c, MVR_E_RCCL, "the communicator of this context was aborted");
  AlignRun run;
  const size_t ns = c->slots[ss].n;
  CurSource cur(c, ss, false, true);
  // Everything that can fail for LOCAL reasons is reported through the iteration's collectives (neutral keys, a zero row, a failure
  // count of 1), so that every rank leaves the iteration together (the set-up below and the transform inside the loop
  // used to return at once, leaving the peers to wait_timeout_ms).  Only the two buffers the collectives themselves run on have
  // to exist for that: a rank that cannot even allocate those cannot report, and its peers leave through the timeout.
  if (int rc = ensure(c, c->seq_keys, c->seq_keys_cap, std::max<size_t>(ns, 1))) return rc;
  if (!c->seq_row) MVR_HIP_TRY(c, hipMalloc(&c->seq_row, 40 * sizeof(double)));
  int carry = cur.start_on_scratch();
  Criteria crit(p);
  Cloud &tgt = c->slots[ts];
  do {
    int local = carry;          // (a failure of the set-up, or of the transform that ended the iteration before)
    if (local == MVR_OK && c->inject_fail_at >= 0 && c->dist_pass == c->inject_fail_at) local = set_error(c, MVR_E_HIP, "injected failure of this rank's local work");
    ++c->dist_pass;
    if (local == MVR_OK) local = forward_keys_impl(c, *cur, tgt, p->max_corr_dist, p->fma_dist, c->seq_keys);
    if (local != MVR_OK && ns) (void)hipMemsetAsync(c->seq_keys, 0x7F, ns * sizeof(long long), c->stream);      // "no neighbour here" (any key above every real one)
    if (ns) { if (int rc = comm_allreduce(c, c->seq_keys, ns, kReduceMinI64)) return rc; }
    if (local == MVR_OK) local = moments2_from_keys_impl(c, *cur, tgt, c->seq_keys, p->max_corr_dist, p->use_reciprocal, p->fma_dist, origin, c->seq_row);
    // [32] of the row counts the ranks whose local work failed in this iteration
    c->h_moments[48] = local == MVR_OK ? 0.0 : 1.0;
    if (local != MVR_OK) (void)hipMemsetAsync(c->seq_row, 0, 32 * sizeof(double), c->stream);
    MVR_HIP_TRY(c, hipMemcpyAsync(c->seq_row + 32, c->h_moments + 48, sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (int rc = comm_allreduce(c, c->seq_row, 33, kReduceSumF64)) return rc;
    MVR_HIP_TRY(c, hipMemcpyAsync(c->h_moments, c->seq_row, 33 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (int rc = stream_wait(c)) return rc;
    const double *h = c->h_moments;
    if (h[32] > 0.0) return local != MVR_OK ? local : set_error(c, MVR_E_RCCL, "a peer's local work failed in this iteration");
    run.fwdq += (double)ns;
    run.ncorr = (int)std::llround(h[0]);
    if (h[0] < 3.0) { run.fail(MVR_E_NOCORR); break; }
    mvr_pair_moments2_t m2;
    std::memset(&m2, 0, sizeof m2);
    m2.n = h[0];
    for (int k = 0; k < 3; ++k) { m2.origin[k] = origin[k]; m2.sp[k] = h[4 + k]; m2.sq[k] = h[7 + k]; }      // (the origin is a constant, not a sum over ranks)
    for (int k = 0; k < 6; ++k) { m2.spp[k] = h[10 + k]; m2.sqq[k] = h[16 + k]; }
    for (int k = 0; k < 9; ++k) m2.spq[k] = h[22 + k];
    m2.sum_d2 = h[31];
    mvr_pair_moments_t mom;
    if (int rc = mvr_moments_from_moments2(&m2, &mom)) return set_error(c, rc, "moments of the sharded align");
    if (int rc = mvr_umeyama_from_moments(&mom, run.tr, nullptr)) return set_error(c, rc, "Umeyama of the sharded align");
    run.cur_mse = h[31] / h[0];                          // mean of the correspondences' (f32) squared distances, as PCL has it
    carry = cur.move(run.tr);          // (reported through the NEXT iteration's collectives, if there is one)
    run.compose();
    run.converged = crit.converged(run.tr, run.cur_mse, run.iters, &run.state) ? 1 : 0;
  } while (!run.converged);
  if (carry != MVR_OK) return carry;
  return run.finish(c, os, ss, false, T_out, st);      // (the sharded align has no normals)
}

// ---- the sequential drivers: what both have in common
namespace {
// the three working slots and the views' slots are all different
bool seq_slots_ok(int n_views, const int *raw_slots, int target_slot, int source_slot, int out_slot)
{
  if (!slot_ok(target_slot) || !slot_ok(source_slot) || !slot_ok(out_slot) || target_slot == source_slot || target_slot == out_slot || source_slot == out_slot)
    return false;
  for (int v = 0; v < n_views; ++v)
    if (!slot_ok(raw_slots[v]) || raw_slots[v] == target_slot || raw_slots[v] == source_slot || raw_slots[v] == out_slot) return false;
  return true;
}

// registrator.cpp:530-541: views 1, V-1, 2, V-2, ..., V/2
std::vector<int> seq_view_order(int n_views)
{
  std::vector<int> order;
  for (int i = 1; i < n_views / 2; ++i) { order.push_back(i); order.push_back(n_views - i); }
  if (n_views / 2 >= 1 && (order.empty() || order.back() != n_views / 2)) order.push_back(n_views / 2);
  return order;
}

// one align of view v is done: its entry in the caller's log, and pose_v <- T_icp * pose_v (registrator.cpp:573-574)
void seq_record(int *done, int v, const float T[16], const mvr_icp_stats &st, double *poses, int *align_view, float *align_T,
                mvr_icp_stats *align_stats, int *n_aligns)
{
  if (align_view) align_view[*done] = v;
  if (align_T) std::memcpy(align_T + 16 * (size_t)*done, T, 16 * sizeof(float));
  if (align_stats) align_stats[*done] = st;
  ++*done;
  if (n_aligns) *n_aligns = *done;
  double Td[16], P[16];
  for (int k = 0; k < 16; ++k) Td[k] = (double)T[k];
  mvr_mat4d_mul(Td, poses + 16 * (size_t)v, P);
  std::memcpy(poses + 16 * (size_t)v, P, sizeof P);
}
}  // namespace

// Registrator::registrationICP (registrator.cpp:526-588) with the growing target sharded over the ranks: view order
// 1, V-1, 2, ..., each view aligned against everything merged so far, pose_v <- T_icp * pose_v (:574), and
// `*target += transformed_source` (:576) as "every rank appends ITS slice of the aligned scan to its shard".
// Rank g of G owns points [n g / G, n (g + 1) / G) of every merged scan; global point numbers run scan after scan in
// merge order.  All ranks call this with the same arguments and get the same poses and logs.
API int mvr_seq_run_sharded(mvr_ctx *ctx, int n_views, const int *raw_slots, int target_slot, int source_slot, int out_slot,
                            const mvr_icp_params *p, const double origin[3], int repeat, double *poses, int *align_view, float *align_T,
                            mvr_icp_stats *align_stats, int *n_aligns)
{
  if (!ctx || n_views < 2 || !raw_slots || !p || !origin || !poses || repeat < 0) return MVR_E_ARG;
  if (!seq_slots_ok(n_views, raw_slots, target_slot, source_slot, out_slot)) return MVR_E_ARG;
  Ctx *c = CTX(ctx);
  MVR_HIP_TRY(c, hipSetDevice(c->device));
  const size_t G = (size_t)(c->comm ? c->comm_world : 1), g = (size_t)(c->comm ? c->comm_rank : 0);
  const std::vector<int> order = seq_view_order(n_views);
  int done = 0;
  if (n_aligns) *n_aligns = 0;
  for (int r = 0; r < repeat; ++r) {
    // target <- this rank's slice of the posed view 0
    size_t n0 = c->slots[raw_slots[0]].n, base = 0;
    if (int rc = mvr_cloud_transform(ctx, out_slot, raw_slots[0], poses)) return rc;
    if (int rc = mvr_cloud_clear(ctx, target_slot)) return rc;
    {
      const size_t lo = n0 * g / G, hi = n0 * (g + 1) / G;
      if (int rc = mvr_cloud_append_range(ctx, target_slot, out_slot, lo, hi - lo, base + lo)) return rc;
    }
    base += n0;
    for (int v : order) {
      if (int rc = mvr_cloud_transform(ctx, source_slot, raw_slots[v], poses + 16 * (size_t)v)) return rc;
      float T[16];
      mvr_icp_stats st;
      std::memset(&st, 0, sizeof st);
      const int rc = mvr_seq_align_sharded(ctx, source_slot, target_slot, out_slot, p, origin, T, &st);
      if (rc != MVR_OK && rc != MVR_E_NOCORR) return rc;      // (PCL's "not enough correspondences": the driver goes on, registrator.cpp:569-574)
      seq_record(&done, v, T, st, poses, align_view, align_T, align_stats, n_aligns);
      const size_t nv = c->slots[out_slot].n, lo = nv * g / G, hi = nv * (g + 1) / G;
      if (int rc2 = mvr_cloud_append_range(ctx, target_slot, out_slot, lo, hi - lo, base + lo)) return rc2;
      base += nv;
    }
  }
  return MVR_OK;
}

// Registrator::registrationICP (registrator.cpp:526-588) on ONE GPU, as one native call: `repeat` sweeps, each posing view 0 into
// the model, then views 1, V-1, 2, ... aligned against everything merged so far (mvr_icp_align), pose_v <- T_icp * pose_v (:574)
// and `*target += aligned source` (:576).  What a host language's loop over the same calls does (include/mvr/registrator.hpp:
// registrationICPDevice; tests / bench: Python), without that language between the calls.  reserve_points: the model's final
// size if known (0: the sum of the scans), reserved once so that the model grows in place.
API int mvr_seq_run(mvr_ctx *ctx, int n_views, const int *raw_slots, int target_slot, int source_slot, int out_slot,
                    const mvr_icp_params *p, int repeat, double *poses, int *align_view, float *align_T, mvr_icp_stats *align_stats,
                    int *n_aligns)
{
  if (!ctx || n_views < 2 || !raw_slots || !p || !poses || repeat < 0) return MVR_E_ARG;
  if (!seq_slots_ok(n_views, raw_slots, target_slot, source_slot, out_slot)) return MVR_E_ARG;
  Ctx *c = CTX(ctx);
  MVR_HIP_TRY(c, hipSetDevice(c->device));
  const std::vector<int> order = seq_view_order(n_views);
  size_t total = 0;
  for (int v = 0; v < n_views; ++v) total += c->slots[raw_slots[v]].n;
  int done = 0;
  if (n_aligns) *n_aligns = 0;
  for (int r = 0; r < repeat; ++r) {
    if (int rc = mvr_cloud_transform(ctx, target_slot, raw_slots[0], poses)) return rc;       // :562
    if (int rc = mvr_cloud_reserve(ctx, target_slot, total)) return rc;
    for (int v : order) {
      // (the model grew by the previous align's output: the launch that poses this source refreshes the model's tail on the way)
      c->refresh_rider = c->seq_rider ? &c->slots[target_slot] : nullptr;
      const int rct = mvr_cloud_transform(ctx, source_slot, raw_slots[v], poses + 16 * (size_t)v);              // :565
      c->refresh_rider = nullptr;
      if (rct != MVR_OK) return rct;
      float T[16];
      mvr_icp_stats st;
      std::memset(&st, 0, sizeof st);
      const int rc = mvr_icp_align(ctx, source_slot, target_slot, out_slot, p, T, &st);                          // :566-569
      if (rc != MVR_OK && rc != MVR_E_NOCORR) return rc;      // (PCL's "not enough correspondences": the driver goes on, registrator.cpp:569-574)
      seq_record(&done, v, T, st, poses, align_view, align_T, align_stats, n_aligns);                           // :573-574
      if (int rc2 = mvr_cloud_append(ctx, target_slot, out_slot)) return rc2;                                    // :576
    }
  }
  return MVR_OK;
}
