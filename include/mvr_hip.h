/*
 * include/mvr_hip.h -- C-ABI of the MI355X-native ICP hot path (libmvr_hip.so).
 *
 * The reference (fanxiaochen/Multi-View-Registration, `mvr`) has no FFI or
 * plugin interface for this path: the boundary is the set of PCL member
 * functions that Registrator calls.  Each entry point
 * below names the reference call site(s) it stands behind; the C++ shim in
 * include/mvr/ (source-compatible PCL-style classes) is the only intended
 * caller, and INTEGRATION.md shows the binding a maintainer would add.
 *
 * Conventions
 *  - plain C types only; every function returns 0 (MVR_OK) or a negative
 *    mvr_status; no exceptions cross this boundary.
 *  - points are 16-byte records {x,y,z,w} (pcl::PointXYZ layout,
 *    mvr/include/types.h:14) or packed 12-byte xyz; `stride_bytes` says which.
 *    Uploads COPY: the caller keeps ownership and may mutate or alias its
 *    clouds between calls, as the reference does (registrator.cpp:576, :920).
 *  - poses are 4x4 column-major, column-vector convention: the memory layout
 *    of Eigen::Matrix4f (what icp.getFinalTransformation() returns,
 *    registrator.cpp:573).  mvr/include/types.h:20-50 (PclMatrixCaster) is the
 *    transposing bridge to OSG's row-vector matrices.
 *  - one mvr_ctx per host thread and GPU; a ctx is not thread-safe (the
 *    reference drives the path from one worker thread, registrator.cpp:606).
 *  - clouds live in numbered device "slots" of the ctx.
 *  - the library fails loudly: with no usable GPU mvr_ctx_create returns
 *    MVR_E_HIP; there is NO CPU fallback anywhere behind this header.
 */
#ifndef MVR_HIP_H
#define MVR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mvr_ctx mvr_ctx;

typedef enum {
  MVR_OK        =  0,
  MVR_E_ARG     = -1,   /* bad argument / slot / size                       */
  MVR_E_HIP     = -2,   /* HIP runtime error or no GPU (see mvr_last_error) */
  MVR_E_NOCORR  = -3,   /* < 3 correspondences (PCL min_number_correspondences_ = 3;
                           "Not enough correspondences found", App. A.1)   */
  MVR_E_NOMEM   = -4,
  MVR_E_SINGULAR= -5,   /* singular system in a host solve (LUM)            */
  MVR_E_RCCL    = -6    /* RCCL failure, or librccl not loadable (multi-GPU entry points only) */
} mvr_status;

#define MVR_MAX_SLOTS 256

/* ---- parameters of one IterativeClosestPoint::align ----------------------
 * Setters at mvr/src/registrator.cpp:551-560, :768-771, :901-904.           */
typedef struct {
  int    use_reciprocal;          /* setUseReciprocalCorrespondences(bool)  */
  double max_corr_dist;           /* setMaxCorrespondenceDistance(double)   */
  int    max_iterations;          /* setMaximumIterations(int)              */
  double transformation_epsilon;  /* setTransformationEpsilon(double)       */
  double euclidean_fitness_eps;   /* setEuclideanFitnessEpsilon(double)     */
  int    fma_dist;                /* 0 (spec): d2 = (dx*dx+dy*dy)+dz*dz, each op
                                     rounded (FLANN L2_Simple); 1: fma chain */
  int    point_to_plane;          /* 0 (the reference): TransformationEstimationSVD;
                                     1 (EXTENSION, BASELINE config 2; no counterpart in
                                     the reference): PCL's point-to-plane LLS estimator on
                                     the same correspondences; needs target normals */
} mvr_icp_params;

/* pcl::registration::DefaultConvergenceCriteria::ConvergenceState */
enum { MVR_CONV_NOT = 0, MVR_CONV_ITERATIONS = 1, MVR_CONV_TRANSFORM = 2,
       MVR_CONV_ABS_MSE = 3, MVR_CONV_REL_MSE = 4, MVR_CONV_NO_CORRESPONDENCES = 5 };

typedef struct {
  int    iterations;   /* nr_iterations_                                    */
  int    converged;    /* hasConverged()                                    */
  int    state;        /* MVR_CONV_*                                        */
  int    n_corr;       /* accepted correspondences, last iteration          */
  double mse;          /* mean squared correspondence distance, last iter.  */
  double evals;        /* point-pair distance evaluations performed (fwd + reciprocal) */
  double fwd_queries;  /* source queries of the forward NN passes           */
  double ms;           /* wall milliseconds spent inside the call           */
} mvr_icp_stats;

/* moments of one scan pair under its accepted correspondences (K5+K6):
 * what TransformationEstimationSVD accumulates (App. A.3).                 */
typedef struct {
  double n;            /* M = number of accepted correspondences           */
  double mean_src[3];  /* (1/M) sum p_i                                     */
  double mean_tgt[3];  /* (1/M) sum q_i                                     */
  double mse;          /* (1/M) sum d2_i                                    */
  double sigma[9];     /* (1/M) sum (q_i-mean_tgt)(p_i-mean_src)^T, row-major */
} mvr_pair_moments_t;

/* raw second moments of one scan pair (K8): everything LUM::computeEdge needs
 * for ANY pair of vertex poses (see mvr_lum_edge_from_moments).  Points are
 * taken relative to `origin` to keep magnitudes small.                     */
typedef struct {
  double n;
  double origin[3];
  double sp[3], sq[3];        /* sum p, sum q                               */
  double spp[6], sqq[6];      /* sum p p^T, sum q q^T : xx xy xz yy yz zz   */
  double spq[9];              /* sum p q^T, row-major                       */
  double sum_d2;              /* sum of the accepted correspondences' squared distances (the f32 values the search
                                 found, added in f64): the pair's residual; 0 when the caller supplied the pairs */
} mvr_pair_moments2_t;       /* 32 doubles: exactly one row of the device edge table */

/* ---- context -------------------------------------------------------------- */
int  mvr_ctx_create(mvr_ctx **ctx, int device_id);
/* as above, but all work is enqueued on `hip_stream` (a hipStream_t owned by
 * the caller, e.g. torch.cuda.current_stream().cuda_stream) instead of a
 * private stream; NULL = private stream. */
int  mvr_ctx_create_on_stream(mvr_ctx **ctx, int device_id, void *hip_stream);
int  mvr_ctx_destroy(mvr_ctx *ctx);
int  mvr_ctx_sync(mvr_ctx *ctx);                 /* wait for the ctx stream   */
const char *mvr_strerror(int status);
const char *mvr_last_error(const mvr_ctx *ctx);  /* detail of the last failure */
int  mvr_device_info(mvr_ctx *ctx, char *name, size_t name_cap, int *n_cu, int *clock_mhz);

/* ---- clouds ----------------------------------------------------------------
 * setInputSource/setInputTarget (registrator.cpp:566-567, 497-498, 645-646,
 * 776-777, 913-914) and lum.addPointCloud (:636) become an upload into a slot. */
int  mvr_cloud_upload(mvr_ctx *ctx, int slot, const float *xyz, size_t n, size_t stride_bytes);
int  mvr_cloud_download(mvr_ctx *ctx, int slot, float *xyz, size_t cap_points, size_t stride_bytes, size_t *n);
int  mvr_cloud_size(mvr_ctx *ctx, int slot, size_t *n);
int  mvr_cloud_reserve(mvr_ctx *ctx, int slot, size_t capacity_points);
int  mvr_cloud_copy(mvr_ctx *ctx, int dst_slot, int src_slot);
/* `*target += transformed_source` (registrator.cpp:576, :833, :982). */
int  mvr_cloud_append(mvr_ctx *ctx, int dst_slot, int src_slot);
int  mvr_cloud_clear(mvr_ctx *ctx, int slot);
/* PointCloud::denoise(segment_threshold, triangle_length) (mvr/src/point_cloud.cpp:423-465): link the points
 * whose distance is <= triangle_length (the same connected components as the reference's Delaunay edges of that
 * length: the Euclidean MST is a subgraph of the Delaunay triangulation), drop the components with fewer than
 * segment_threshold points; the cloud in `slot` is replaced by the kept points, component after component (ordered
 * by their smallest point index), points in index order -- the reference's output order.  kept_index (optional,
 * host, capacity = old size) receives the original indices of the kept points.  One documented difference: exact
 * duplicate points are ordinary members of their component here, while CGAL's insert keeps only the first of them as a
 * vertex (the later copies become isolated and are dropped by any segment_threshold > 1).
 * Distances: sqrt(dx*dx + dy*dy + dz*dz) in f64 from the f32 coordinates, each operation rounded; a pair is linked when
 * `!(d > triangle_length)`, so d == triangle_length links.  segment_threshold <= 0 keeps everything.  triangle_length may be
 * 0 (exact duplicates link, nothing else) or +inf (one component of all finite points); NaN or < 0 returns MVR_E_ARG and
 * changes nothing.  Normals of the slot follow their points.  The output is a NEW point set, also when nothing is kept.
 * Non-finite points (a NaN or an infinity in x, y or z; w is not looked at), worded like N1-N5 of mvr_knn and rule 2 of
 * the outlier filters:
 *  D1. Such a point is linked to nothing, whatever triangle_length is (+inf included: two points at the same infinite
 *      coordinates are not linked either).
 *  D2. It is a component of its own, of size 1: counted in n_components, kept exactly when segment_threshold <= 1, at its
 *      place in the (smallest index of the component, index) order like any other point.
 *  D3. It takes no part in the sizing of the grid: the cells are sized by the finite points alone, so the cost of a call
 *      does not depend on where the non-finite coordinates are.
 *  D4. A cloud with no finite point is sized like a single point: n components of size 1, MVR_OK. */
int  mvr_cloud_denoise(mvr_ctx *ctx, int slot, int segment_threshold, double triangle_length,
                       size_t *n_kept, size_t *n_components, uint32_t *kept_index);
/* ---- voxel-grid downsampling (EXTENSION: pcl::VoxelGrid<PointXYZ>::filter with setLeafSize(lx, ly, lz),
 * setMinimumPointsNumberPerVoxel(min_points) and downsample_all_data = true).  The reference pins no PCL version; where
 * PCL versions differ, or PCL is undefined, the rule below is this library's rule.
 *  1. Finite points only: a point with a non-finite coordinate belongs to no voxel (PCL's is_dense == false path);
 *     min_p / max_p are taken over the finite points.  No finite point (or an empty cloud): empty output, MVR_OK.
 *  2. inv[a] = 1.0f / leaf[a] in f32.  Every leaf[a] must be finite and > 0, else MVR_E_ARG before any GPU work, nothing
 *     changed; MVR_E_ARG too for more than 0xFFFFFFF0 points, a NULL ctx / leaf or a bad slot.
 *  3. PCL's overflow rule: d[a] = (int64)((max_p[a] - min_p[a]) * inv[a]) + 1, the difference and the product in f32.
 *     When d0 * d1 * d2 > INT32_MAX the output is a COPY of the input (every point, non-finite ones included, normals
 *     included), *passthrough = 1 and the call returns MVR_OK.  An axis whose f32 product is not below 2^31 (NaN
 *     included) takes the same exit, and so does an axis where |min_p * inv| or |max_p * inv| is not below 2^62 (PCL's
 *     int cast is undefined there): no cast overflows.  As a last guard, a voxel index (rule 4) that would not fit in 64
 *     bits takes it too; under the bounds above div[a] stays within a small multiple of d[a], so the index needs about 40
 *     bits and this guard does not fire.
 *  4. Voxel index, PCL's f32 arithmetic (the products are f32 multiplies by inv, never contracted):
 *     min_b[a] = floor(min_p[a] * inv[a]), max_b[a] likewise, as integers (64-bit here; PCL's int);
 *     div[a] = max_b[a] - min_b[a] + 1;  ijk[a] = floor(p[a] * inv[a]) - (float)min_b[a], the f32 difference as an
 *     integer (it is a non-negative f32 integer);  idx = ijk0 + ijk1 * div0 + ijk2 * div0 * div1 in 64 bits (where PCL's
 *     int idx can wrap near the limit, this one does not).  A point exactly on a voxel face goes to the upper voxel.
 *  5. A voxel with fewer than min_points points is dropped (0, the default, keeps every occupied voxel).
 *  6. Output points in ascending idx (PCL's order).  voxel_of (optional, host, one entry per SOURCE point): the output
 *     position of point i's voxel; UINT32_MAX for a non-finite point or a dropped voxel; the identity under rule 3.
 *  7. Centroid, per coordinate: the f64 sum of the voxel's f32 coordinates / count, rounded to f32; w = 1.  (PCL sums
 *     in f32; this library deliberately does not.)  Sums run in a fixed order: bit-identical from run to run.
 *  8. Normals: when the source slot carries normals, each output normal is the f64 sum of the voxel's normals,
 *     normalised in f64 (x / sqrt((x*x + y*y) + z*z)) and rounded to f32, w = 0 -- PCL >= 1.8's CentroidPoint /
 *     AccumulatorNormal (PCL 1.7 left the mean unnormalised); normalising keeps the slot's unit-normal rule that
 *     point-to-plane ICP relies on.  A zero sum stays (0, 0, 0); a NaN normal in the voxel gives NaN.  No source
 *     normals: no output normals.
 *  9. dst_slot may equal src_slot (in place); otherwise src_slot is left untouched.  The output is a NEW point set:
 *     orderings, grids and pose bookkeeping are dropped, as after mvr_cloud_upload / mvr_cloud_denoise.
 * n_out / passthrough (optional) receive the output size and the rule-3 flag. */
int  mvr_cloud_voxel_grid(mvr_ctx *ctx, int dst_slot, int src_slot, const float leaf[3], unsigned min_points,
                          size_t *n_out, uint32_t *voxel_of, int *passthrough);
/* PointCloud::getTransformedPoints (point_cloud.cpp:290-303): f32 points times
 * the f64 pose (osg::Matrixd::preMult incl. the w divide), rounded to f32.
 * dst_slot may equal src_slot. */
int  mvr_cloud_transform(mvr_ctx *ctx, int dst_slot, int src_slot, const double T[16]);
/* the same for `count` clouds in ONE launch (the loop over all scans that poses them before a
 * global iteration, registrator.cpp:630-637): T = count x 16 doubles.  The entries run concurrently: a destination
 * slot may not appear twice, nor be the source of ANOTHER entry (MVR_E_ARG); dst[k] == src[k] poses in place.
 * mvr_ring_step / mvr_ring_run hand their posed_slots / raw_slots to this call and inherit the rule. */
int  mvr_cloud_transform_batch(mvr_ctx *ctx, int count, const int *dst_slots, const int *src_slots, const double *T);
/* pcl transformPointCloud / ICP::transformCloud (inside align, App. A.1):
 * x' = ((T00 x + T01 y) + T02 z) + T03 in f32, no contraction. */
int  mvr_cloud_transform_f32(mvr_ctx *ctx, int dst_slot, int src_slot, const float T[16]);
/* EXTENSION (point-to-plane): unit normals of the cloud in `slot`, one per point
 * (n must equal the cloud's size; stride 16 {nx,ny,nz,*} or 12).  Normals follow
 * the cloud through copy / transform (rotated) / append (kept only if both
 * clouds carry normals); a new upload of points drops them. */
int  mvr_cloud_upload_normals(mvr_ctx *ctx, int slot, const float *nxyz, size_t n, size_t stride_bytes);
int  mvr_cloud_download_normals(mvr_ctx *ctx, int slot, float *nxyz, size_t cap_points, size_t stride_bytes, size_t *n);

/* ---- the hot path ------------------------------------------------------------ */
/* exact 1-NN of every point of q_slot in t_slot: tree_->nearestKSearch(p,1,..)
 * (inside icp.align registrator.cpp:569,920,1012,1024 and :502,:649).
 * idx/d2 are host arrays of n_q entries (either may be NULL).  Ties -> lowest
 * index.  idx = UINT32_MAX and d2 = +inf when the target is empty.
 * Non-finite points: no rule.  The index build clamps them into its boxes without converting one to an integer, but what a
 * search returns for a cloud that holds a NaN or an infinity is unspecified and untested; filter such clouds first. */
int  mvr_nn(mvr_ctx *ctx, int q_slot, int t_slot, int fma_dist, uint32_t *idx, float *d2);

/* ---- k nearest neighbours and normal estimation (EXTENSION: pcl::NormalEstimation) -----------------------
 * Distances are the f32 expression of mvr_nn, selected by fma_dist the same way:
 * d2 = (dx*dx + dy*dy) + dz*dz, each operation rounded (fma_dist = 1: the fma chain).
 *
 * k-NN of a query point q in a target cloud T: the k entries of T smallest under the key (d2, index) in
 * lexicographic order, ascending -- ties go to the lower index, as in mvr_nn.  When T holds fewer than k
 * points the tail entries are idx = UINT32_MAX, d2 = +inf (mvr_nn's empty-target convention).  k = 1 gives
 * exactly mvr_nn's (idx, d2), bit for bit.  The search is exact: a uniform grid over T's current
 * coordinates, walked shell by shell until no unvisited cell can hold a point within the k-th d2.
 *
 * Non-finite points (a NaN or an infinity in x, y or z; scanner files with is_dense == false hold them), for mvr_knn and
 * mvr_cloud_estimate_normals alike, with or without fma_dist, for clouds of any size:
 *  N1. A non-finite target point is nobody's neighbour: it is never listed and enters no covariance.  More generally a
 *      pair whose f32 d2 is not finite (which finite points reach only beyond 1e19) is not a neighbour pair.
 *  N2. A non-finite query has no neighbours: idx = UINT32_MAX and d2 = +inf in all k entries.
 *  N3. The tail rule above counts the FINITE target points: with fewer than k of them the tail is UINT32_MAX / +inf.
 *  N4. A non-finite point gets a NaN normal and a NaN curvature; a finite point's normal is that of its finite
 *      neighbours (fewer than 3 of them: NaN, as below).
 *  N5. Non-finite points take no part in the sizing of the grid, and no query walks the grid because of one.
 *  N6. "k = 1 equals mvr_nn" holds for clouds of finite points; mvr_nn has no rule for the others (see there). */
#define MVR_MAX_KNN 64
/* exact k nearest neighbours of every point of q_slot in t_slot; idx / d2 host arrays of n_q * k, row-major
 * (row = query index; either may be NULL).  MVR_E_ARG for k outside 1..MVR_MAX_KNN or a bad slot. */
int  mvr_knn(mvr_ctx *ctx, int q_slot, int t_slot, int k, int fma_dist, uint32_t *idx, float *d2);

/* Normal estimation of a cloud against itself (PCL NormalEstimation::computePointNormal, solvePlaneParameters,
 * flipNormalTowardsViewpoint):
 *  - neighbourhood, k mode: the k-NN list above, the point itself included (d2 = 0);
 *    radius mode: every j with d2(i, j) <= (float)(radius * radius), i included, no cap on the count (PCL
 *    max_nn = 0).  The <= on the f32 d2 is this library's rule: PCL / FLANN were not available to pin theirs.
 *  - fewer than 3 neighbours (k < 3 included): normal = NaN, curvature = NaN, as PCL.
 *  - covariance in f64 of the neighbours' coordinates taken relative to the query point, divided by the
 *    neighbour count.  (Deliberately NOT PCL 1.7's single-pass f32 accumulation, which is less accurate.)
 *  - normal = unit eigenvector of the smallest eigenvalue l0; curvature = |l0| / (l0 + l1 + l2), 0 when the
 *    sum is 0.  A zero covariance (all neighbours at one point) gives some finite unit vector and curvature 0.
 *  - orientation: the normal rounded to f32, cos = dot(vp - p, n) in f32, n negated when cos < 0 (strictly).
 *  - output: the slot's normals ({nx, ny, nz, 0}, what mvr_cloud_upload_normals fills), has_normals set: they
 *    follow the cloud through copy / transform / append / denoise like uploaded normals, point-to-plane ICP and
 *    mvr_cloud_download_normals use them with no host round trip; curvature optionally to the host. */
typedef struct {
  int    k;             /* setKSearch: 1..MVR_MAX_KNN, or 0 for radius mode                      */
  double radius;        /* setRadiusSearch: > 0, or 0 for k mode; exactly one of k / radius set   */
  float  viewpoint[3];  /* setViewPoint (PCL default 0, 0, 0)                                     */
  int    fma_dist;
} mvr_normal_params;
/* normals of `count` slots, each against itself, in one call (one launch for up to 16 slots); curvature: NULL,
 * or `count` host pointers (an entry may be NULL) to arrays of the slot's size.  MVR_E_ARG, before any GPU work,
 * for a NULL ctx / slots / p, both or neither of k / radius set, k > MVR_MAX_KNN, a bad slot or a slot listed
 * twice.  An empty slot is MVR_OK (nothing to do). */
int  mvr_cloud_estimate_normals(mvr_ctx *ctx, int count, const int *slots, const mvr_normal_params *p,
                                float *const *curvature);

/* ---- radius search (EXTENSION: pcl::search::KdTree::radiusSearch) as CSR lists -----------------------------------
 * Every neighbour of every point of q_slot within `radius` in t_slot, as variable-length rows.
 *  RS1. j is a neighbour of query i iff the f32 d2(i, j) <= (float)(radius * radius), that bound kept finite; d2 is the
 *       expression of mvr_nn, or the fma chain with fma_dist.  This is the library's own neighbour rule (rule 14 of the
 *       outlier section, the radius mode of mvr_cloud_estimate_normals, M1, F1, P2 ...): a list returned here IS the
 *       neighbourhood every other radius-mode entry uses.  DEVIATION: FLANN tests a strict < on its own arithmetic, so
 *       a point at exactly the radius is listed here and not there.  With q_slot == t_slot a point is in its own row
 *       (d2 = 0), as in PCL.
 *  RS2. Non-finite points: N1 and N2 of mvr_knn.  A non-finite target point, or a pair whose f32 d2 is not finite, is in
 *       no row; a non-finite query has an empty row; an empty target, or one without a finite point, gives empty rows.
 *  RS3. sorted = 1: a row ascends under the key (d2, index), the key of mvr_knn.  The order is total: exact ties and
 *       duplicates have one answer.
 *  RS4. max_nn > 0: a row holds the min(n_i, max_nn) smallest entries under that key, ALWAYS in the order of RS3,
 *       whatever `sorted` says -- one valid instance of what FLANN may return, and the only deterministic one.  For
 *       max_nn <= MVR_MAX_KNN the row is exactly the prefix of mvr_knn's list with d2 <= r2.
 *  RS5. sorted = 0 and max_nn = 0: the same set per row; the order is unspecified, but identical from call to call with
 *       the same arguments on the same slot state.
 *  RS6. CSR: offsets[i] .. offsets[i + 1] is the row of query INDEX i; offsets[0] = 0, offsets[n_q] = total; idx and d2
 *       are parallel.
 *  RS7. Sizing: offsets (n_q + 1 entries, optional) and *total (optional) are written on every successful count.
 *       idx == NULL && d2 == NULL is a count-only call, `capacity` is ignored.  Otherwise capacity >= total is required:
 *       a short capacity returns MVR_E_ARG with *total and offsets written and no entry written; mvr_last_error names
 *       both numbers.  Either of idx / d2 alone may be NULL.
 *  RS8. A total above MVR_RADIUS_MAX_TOTAL is refused with MVR_E_ARG, *total (and offsets) still written, so that the
 *       caller can split the queries over several slots.  The bound is what the 32-bit item count of the segmented sort
 *       addresses; with max_nn it is also applied to the uncapped lengths of the rows longer than the stage, summed.
 *  RS9. MVR_E_ARG before any GPU work, writing nothing, with mvr_last_error set wherever there is a ctx: a NULL ctx or
 *       params, a bad slot, a radius that is not finite and > 0, a cloud too large for the walks or whose points are not
 *       current.  n_q == 0 is MVR_OK with offsets[0] = 0.
 * RS10. Neither slot is modified: the target gets its own-coordinates grid as in mvr_knn (and the queries theirs, for the
 *       walking order); nothing else about a slot changes.
 * RS11. Results do not depend on the grid's resolution, on the tune key "radius_stage", or on the path a row took.
 * RS12. (internal) radius_search_device leaves offsets / idx / d2 on the device; this entry is that plus the copies home.
 * A row of more than MVR_RADIUS_STAGE entries (tune key "radius_stage", MVR_MAX_KNN..MVR_RADIUS_STAGE, lowers the threshold)
 * is ordered by a segmented radix sort in device memory instead of on chip; mvr_ctx_stat "radius_long_rows" counts them. */
#define MVR_RADIUS_STAGE 1024                /* entries of one row staged and ordered in LDS; above it the long-row path */
#define MVR_RADIUS_MAX_TOTAL 0x7FFFFFFFull   /* RS8 */
typedef struct {
  double   radius;    /* finite, > 0                                                     */
  uint32_t max_nn;    /* 0: no cap (PCL's default); else at most max_nn entries per row  */
  int      sorted;    /* setSortedResults; 1 is PCL's default                            */
  int      fma_dist;
} mvr_radius_params;
void mvr_radius_default_params(mvr_radius_params *p);   /* radius 0 (to be set), max_nn 0, sorted 1, fma_dist 0 */
int  mvr_radius_search(mvr_ctx *ctx, int q_slot, int t_slot, const mvr_radius_params *p,
                       uint64_t *offsets /* n_q + 1, or NULL */, uint32_t *idx, float *d2 /* `capacity` entries each, or NULL */,
                       size_t capacity, size_t *total /* or NULL */);

/* ---- sparse outlier removal (EXTENSION: pcl::StatisticalOutlierRemoval and pcl::RadiusOutlierRemoval) ------------
 * The reference pins no PCL version; where PCL versions differ, or PCL is loose, the rule below is this library's rule.
 * Common to both filters:
 *  1. Distances are the f32 expression of mvr_nn / mvr_knn, d2 = (dx*dx + dy*dy) + dz*dz, each operation rounded;
 *     fma_dist = 1 selects the fma chain.
 *  2. A point with a non-finite coordinate is an outlier by definition: it is nobody's neighbour, enters no statistic,
 *     is never in the inlier output and always in the `negative` output.  (PCL keeps such a point, with a distance of 0;
 *     here, as in mvr_cloud_voxel_grid, a NaN must not reach ICP.)
 *  3. Output: the selected points in their ORIGINAL index order, w = 1; normals of the source slot follow their points.
 *     dst_slot may equal src_slot; otherwise src_slot is left untouched.  The output is a NEW point set: orderings,
 *     grids and pose bookkeeping are dropped, as after mvr_cloud_denoise.
 *  4. negative = 1 (PCL's setNegative(true)) outputs exactly the complement.
 *  5. kept_index (optional, host, capacity = source size) receives the original indices of the output points,
 *     ascending; n_out (optional) their number.
 *  6. An empty cloud is MVR_OK with an empty output.  A NULL ctx / params, a bad slot or a parameter outside its range
 *     (below) returns MVR_E_ARG before any GPU work and writes nothing.
 *
 * Statistical outlier removal (setMeanK, setStddevMulThresh, setNegative):
 *  7. mean_k in 1..MVR_MAX_KNN; stddev_mul any finite double (negative values allowed, as in PCL).
 *  8. For a finite point i take the mean_k smallest d2 over the finite points j != i; other points at the same
 *     location count, at d2 = 0.  (PCL asks for mean_k + 1 neighbours and skips the first: the same multiset.)
 *     mean_dist[i] = f32( (sum, in ascending order of d2, of the correctly rounded f32 sqrt(d2), added in f64) / mean_k ):
 *     PCL's arithmetic.
 *  9. Fewer than mean_k other finite points: no point has a mean distance; every finite point is an inlier,
 *     n_valid = 0, mean / stddev / threshold are NaN and mean_dist is NaN throughout.
 * 10. Statistics over the n_valid finite points in f64, two passes, in a fixed summation order (bit-identical from run
 *     to run): mean = sum(md) / n, stddev = sqrt(sum((md - mean)^2) / (n - 1)), threshold = mean + stddev_mul * stddev.
 *     (PCL's one-pass form (sum(md^2) - sum(md)^2 / n) / (n - 1) can go negative when all distances are equal; this one
 *     cannot.)  n_valid = 1 gives NaN, as PCL.
 * 11. A finite point is an inlier iff !((double)mean_dist[i] > threshold): a NaN threshold keeps every finite point.
 * 12. mean_dist (optional, host, one f32 per SOURCE point): NaN for a non-finite point.  stats (optional).
 *
 * Radius outlier removal (setRadiusSearch, setMinNeighborsInRadius, setNegative):
 * 13. radius finite and > 0; min_neighbors >= 0.
 * 14. count[i] = number of finite j != i with d2(i, j) <= (float)(radius * radius): the rule of the radius mode of
 *     mvr_cloud_estimate_normals, minus the point itself.  A finite point is an inlier iff count[i] >= min_neighbors.
 *     (PCL counts the point itself and removes when k <= min_pts: the same set.)
 * 15. neighbor_count (optional, host, one u32 per SOURCE point): exact, 0 for a non-finite point. */
typedef struct {
  int    mean_k;        /* setMeanK: 1..MVR_MAX_KNN (PCL default 1)            */
  double stddev_mul;    /* setStddevMulThresh (PCL default 0)                  */
  int    negative;      /* setNegative                                         */
  int    fma_dist;
} mvr_sor_params;
typedef struct {
  double mean, stddev, threshold;   /* of the mean distances (rule 10)         */
  size_t n_valid;                   /* points that have a mean distance        */
} mvr_sor_stats;
typedef struct {
  double radius;        /* setRadiusSearch: finite, > 0                        */
  int    min_neighbors; /* setMinNeighborsInRadius: >= 0 (PCL default 1)       */
  int    negative;      /* setNegative                                         */
  int    fma_dist;
} mvr_ror_params;
int  mvr_cloud_statistical_outlier_removal(mvr_ctx *ctx, int dst_slot, int src_slot, const mvr_sor_params *p, size_t *n_out,
                                           uint32_t *kept_index, float *mean_dist, mvr_sor_stats *stats);
int  mvr_cloud_radius_outlier_removal(mvr_ctx *ctx, int dst_slot, int src_slot, const mvr_ror_params *p, size_t *n_out,
                                      uint32_t *kept_index, uint32_t *neighbor_count);

/* ---- moving-least-squares smoothing (EXTENSION: pcl::MovingLeastSquares) -----------------------------------------
 * The reference pins no PCL version; where PCL versions differ, or PCL is loose, the rule below is this library's rule.
 * The model is PCL's computeMLSPointNormal with upsampling NONE and the SIMPLE projection; deviations are marked.
 *  M1. Neighbourhood: point i's neighbours are every finite j with d2(i, j) <= (float)(radius * radius) under the f32
 *      distance of mvr_nn / mvr_knn, i itself included -- exactly the radius mode of mvr_cloud_estimate_normals;
 *      fma_dist = 1 selects the fma chain.
 *  M2. A non-finite point is nobody's neighbour and is never in the output, and no query walks the grid because of one
 *      (rules N1, N2 and N5 above).
 *  M3. A finite point with fewer than 3 neighbours is dropped, as PCL does.  The output holds the other points in their
 *      ORIGINAL index order, w = 1.  kept_index (optional, host, capacity = source size) receives the original indices,
 *      ascending; n_out (optional) their number; curvature (optional, host) one f32 per OUTPUT point.
 *  M4. Plane: the f64 mean and covariance of the neighbours' coordinates taken relative to the query point, divided by
 *      the count (the arithmetic of mvr_cloud_estimate_normals; deliberately NOT PCL's f32 accumulation).  n = unit
 *      eigenvector of the smallest eigenvalue l0.  The projected query is q' = q - ((q - mean) . n) n;
 *      curvature = |l0| / (l0 + l1 + l2), 0 when the sum is 0.
 *  M5. Polynomial: applies iff order == 2 and the neighbour count is at least 6 (PCL's polynomial_fit = order > 1).
 *      With any orthonormal pair u, v such that u x v = n (the result does not depend on the choice: the polynomials of
 *      total degree 2 are closed under rotation and the weights are radial), every neighbour p gives d = p - q',
 *      (a, b, f) = (d . u, d . v, d . n) and w = exp(-(d . d) / sqr_gauss_param), all in f64 -- the distance from the
 *      PROJECTED point, as PCL recomputes it.  The normal equations are those of the basis 1, b, b^2, a, ab, a^2 (PCL's
 *      coefficient order c0..c5): 15 distinct monomial sums and 6 right-hand sums, solved by Cholesky in f64.  A pivot that
 *      is not finite and positive, or a coefficient c0 / c1 / c3 that is not finite (a pivot can be positive and as small as
 *      a denormal), abandons the fit and the plane result of M4 stands (PCL: an LLT solve whose result it
 *      does not check).  On success q'' = q' + c0 n and, with compute_normals, the normal is
 *      normalize(n - c3 u - c1 v).
 *  M6. Output coordinates are the f64 result rounded to f32.  A computed normal is {nx, ny, nz, 0}: the unit vector rounded
 *      to f32, then oriented with the f32 test of mvr_cloud_estimate_normals (negated when cos < 0, strictly) -- orient 0:
 *      cos = dot(viewpoint - p, n) with p the SOURCE point; orient 1: cos = dot(source normal of the same point, n).  (PCL
 *      leaves the eigenvector's sign as it falls.)  Without compute_normals the source slot's normals follow their points
 *      unchanged, as in the outlier filters; no source normals and no compute_normals: no output normals.
 *  M7. dst_slot may equal src_slot: every read comes from the source as it was before the call.  Otherwise src_slot is left
 *      untouched.  The output is a NEW point set: orderings, grids and pose bookkeeping are dropped.
 *  M8. MVR_E_ARG, before any GPU work and with nothing written, for a NULL ctx / params, a bad slot, a radius or
 *      sqr_gauss_param that is non-finite or negative, a radius of 0, an order outside 0..2, an orient outside 0..1, a
 *      non-finite viewpoint, orient 1 on a source slot without normals, a cloud above 0x7FFFFFF0 points, or a cloud whose
 *      points are stale because a pipelined run is in flight.  An empty cloud is MVR_OK with an empty output.
 *  M9. Bit-identical from run to run on one grid: one thread per query, sums in walk order, no atomics.
 * Out of scope: PCL's upsampling methods (SAMPLE_LOCAL_PLANE, RANDOM_UNIFORM_DENSITY, VOXEL_GRID_DILATION, DISTINCT_CLOUD),
 * the ORTHOGONAL projection, polynomial orders above 2 and per-point polynomial caching (setCacheMLSResults). */
typedef struct {
  double radius;           /* setSearchRadius: finite, > 0                                                              */
  int    order;            /* setPolynomialOrder: 0..2; below 2 the plane projection alone (PCL's polynomial_fit = order > 1) */
  double sqr_gauss_param;  /* setSqrGaussParam: finite, > 0; 0 selects PCL's default radius * radius                       */
  int    compute_normals;  /* setComputeNormals                                                                           */
  int    orient;           /* 0: towards `viewpoint` (the flip rule of mvr_cloud_estimate_normals);
                              1: along the source slot's own normals (MVR_E_ARG when it has none)                          */
  float  viewpoint[3];
  int    fma_dist;
} mvr_mls_params;
int  mvr_cloud_mls(mvr_ctx *ctx, int dst_slot, int src_slot, const mvr_mls_params *p, size_t *n_out,
                   uint32_t *kept_index, float *curvature);

/* ---- fast point feature histograms (EXTENSION: pcl::FPFHEstimation) ----------------------------------------------------
 * The 33-bin signatures a feature matcher or a sample-consensus aligner starts from when no pose prior is at hand.  The
 * reference pins no PCL version; the model is pcl/features/impl/fpfh.hpp (computePointSPFHSignature,
 * weightPointSPFHSignature) and pcl::computePairFeatures in radius mode; deviations are marked.
 *  F1. Input: the cloud in `slot` and its normals; the cloud is search surface and input at once (PCL: setSearchSurface
 *      unset, all indices).  A point is VALID when its three coordinates and its three normal components are finite.  An
 *      invalid point is nobody's neighbour and enters no count and no sum; its own signature and its SPFH row are 33 NaN and
 *      its neighbor_count is 0; no query walks the grid because of one (rules N2 and N5 above).
 *  F2. Neighbourhood: N(i) = every valid j with d2(i, j) <= (float)(radius * radius) under the f32 distance of mvr_nn /
 *      mvr_knn, i itself included -- exactly the radius mode of mvr_cloud_estimate_normals; fma_dist = 1 selects the fma
 *      chain.  n_i = |N(i)|.
 *  F3. Pair features of (i, j), j in N(i), j != i, all in f32, every operation rounded, none contracted.  A dot product is
 *      (ax*bx + ay*by) + az*bz, a norm sqrtf of that.  dp = p_j - p_i, f4 = |dp|; f4 == 0: no features (PCL returns false).
 *      a1 = (n_i . dp) / f4, a2 = (n_j . dp) / f4.  Swap iff fabsf(a1) < fabsf(a2): the roles of n_i and n_j exchange,
 *      dp = -dp and f3 = -a2; otherwise f3 = a1.  (PCL tests acos(|a1|) > acos(|a2|): the same wherever f32 acos is
 *      injective, without the libm call.)  With n1 / n2 the normals after the swap: v = dp x n1; |v| == 0: no features;
 *      v /= |v|; w = n1 x v; f2 = v . n2; f1 = atan2f(w . n2, n1 . n2).
 *  F4. Bins, PCL's expressions in f64 from the f32 feature: b1 = floor(11 * ((f1 + M_PI) * (double)d_pi)) with
 *      d_pi = (float)(1 / (2 pi)); b2 = floor(11 * ((f2 + 1.0) * 0.5)), b3 the same from f3; each clamped to 0..10.
 *  F5. SPFH: c_i[f][b] = the number of pairs of i that F3 gives features and F4 puts in bin b of feature f, an exact integer;
 *      SPFH_i[f][b] = (float)c * (100.0f / (float)(n_i - 1)) in f32; n_i = 1: 33 zeros.  Pairs without features still count
 *      in n_i - 1, as in PCL.  (PCL adds the increment 100 / (n_i - 1) c times in f32: a difference of rounding only.)
 *  F6. FPFH: for every j in N(i) with d2 != 0 and w = 1.0f / d2 finite, val = SPFH_j[f][b] * w in f32 (PCL's arithmetic: the
 *      weight is one over the SQUARED distance) is added in f64 to the bin and to the sum of its feature, in walk order; the
 *      query's own SPFH is not added, as in PCL.  Output (float)(bin * (100.0 / sum_f)) when sum_f != 0, else 0: each of the
 *      three 11-bin blocks of a point with a contributing neighbour sums to 100.  (PCL accumulates the bins in f32 in the
 *      order FLANN returns the neighbours; here the order is the grid walk's and the sums are f64.)
 *  F7. MVR_E_ARG, before any GPU work and with nothing written, for a NULL ctx / params, a bad slot, a radius that is
 *      non-finite or <= 0, a slot without normals, a cloud above 0x7FFFFFF0 points, or a cloud whose points are stale
 *      because a pipelined run is in flight.  An empty cloud is MVR_OK.  All three outputs NULL: MVR_OK after the work.
 *  F8. Bit-identical from run to run on one grid: one thread per query, one fixed walk order, no floating-point atomics.
 * The slot is not modified and no descriptor stays on the device after the call.
 * Out of scope: the k-neighbour mode (setKSearch).  setSearchSurface / setIndices are mvr_cloud_fpfh_at below (rules Q1-Q8), PFH
 * is mvr_cloud_pfh below.  The
 * matching and the sample-consensus alignment that consume the signatures follow below (mvr_feature_knn,
 * mvr_align_prerejective). */
#define MVR_FPFH_BINS 11            /* per feature; a signature is 3 * 11 = 33 floats (pcl::FPFHSignature33) */
typedef struct {
  double radius;        /* setRadiusSearch: finite, > 0 */
  int    fma_dist;
} mvr_fpfh_params;
int  mvr_cloud_fpfh(mvr_ctx *ctx, int slot, const mvr_fpfh_params *p,
                    float *fpfh,              /* host, n * 33, row = point index; may be NULL   */
                    float *spfh,              /* optional host, n * 33: the intermediate SPFH   */
                    uint32_t *neighbor_count  /* optional host, n: n_i of rule F2               */);

/* ---- point feature histograms (EXTENSION: pcl::PFHEstimation) -----------------------------------------------------------
 * The 125-bin descriptor FPFH approximates: the joint histogram of the three angular features over EVERY pair of a
 * neighbourhood, n_i (n_i - 1) / 2 pairs per point.  PCL was not at hand; the model is pcl/features/impl/pfh.hpp
 * (computePointPFHSignature, computeFeature) with nr_subdiv = 5, as published; deviations are marked.
 *  P1. Input and validity: rule F1.  The cloud in `slot` is input and search surface at once, with its normals.  A point is
 *      VALID when its three coordinates and its three normal components are finite.  An invalid point gets 125 NaN and
 *      neighbor_count 0 and is nobody's neighbour.
 *  P2. Neighbourhood: exactly one of radius / k is set.  Every n_i is allowed: no on-chip capacity caps it (P6 aside).
 *      Radius mode: N(i) is rule F2 -- the f32 distance, fma_dist as everywhere, i itself included.
 *      k mode (1 <= k <= MVR_MAX_KNN; offered here, PCL's setKSearch): N(i) = the listed entries of mvr_knn's list of i in its
 *      own cloud (rules N1-N3, key = (d2 bits, index)) minus the entries whose normal is not finite -- whether or not i itself
 *      is among them (duplicates with lower indices can push it out).  n_i = |N(i)|.
 *  P3. Pairs: every unordered pair {a, b} of N(i) is counted once.  N(i) is ordered by the key (bits of the f32 d2 to the
 *      query, index), ascending -- PCL's list order when FLANN returns sorted lists, ties aside -- and the pair features are
 *      rule F3, verbatim and in the same f32 arithmetic (one piece of code serves both descriptors), with the LATER member of
 *      the pair in F3's role of "i" and the EARLIER in the role of "j": PCL calls computePairFeatures(indices[i_idx],
 *      indices[j_idx]) with j_idx < i_idx.  Nothing is sorted: a pair compares its two keys.
 *  P4. Bins: F4 with 5 in place of 11: b1, b2, b3 in 0..4; the joint bin is h = b1 + 5 * b2 + 25 * b3.
 *  P5. Histogram: c_i[h] = the number of pairs that P3 gives features and P4 puts in h, an exact unsigned integer;
 *      m_i = n_i (n_i - 1) / 2 in 64 bits; out[h] = (float)c * (100.0f / (float)m_i) in f32.  (PCL adds the increment c times
 *      in f32: a difference of rounding only.)  Pairs without features (f4 == 0 or |v| == 0) still count in m_i, as in PCL.
 *      n_i == 1: 125 zeros.  n_i == 0 (k mode only): 125 NaN, PCL's "no neighbours".
 *  P6. Range: a query with n_i > 65 535 makes the call fail with MVR_E_ARG, nothing written; the neighbourhoods are counted
 *      before any such query's pairs are.  DEVIATION: PCL has no such limit (and would need days for such a point).
 *  P7. MVR_E_ARG, before any GPU work and with nothing written, for everything F7 lists, for both or neither of radius / k
 *      set (radius: finite and > 0, or 0; k: 1..MVR_MAX_KNN, or 0).  An empty cloud is MVR_OK.  All three outputs NULL:
 *      MVR_OK after the work.
 *  P8. The counts are integers added with integer atomics, so the result does not depend on the order of the pairs, on which
 *      lane computes which, on the resolution of the grid or on any tune key: bit-identical from run to run, from grid to
 *      grid, and between the staged and the tiled path.  No floating-point atomics anywhere.
 * One wave per query: it walks the ball over the cloud's own grid with its lanes over the cells' rows (k mode: it reads the k
 * list), stages the neighbours in LDS, deals the pairs over its 64 lanes and counts into a 125-bin u32 histogram in LDS.  A
 * neighbourhood of more than MVR_PFH_STAGE points (tune key "pfh_stage", MVR_MAX_KNN..MVR_PFH_STAGE, lowers the threshold)
 * goes to device scratch and is processed tile against tile.  mvr_ctx_stat "pfh_tiled_queries" / "pfh_pairs": the queries of
 * the last call that took the tiled path, and its sum of m_i.
 * The slot is not modified and nothing stays on the device after the call.
 * setSearchSurface / setIndices are mvr_cloud_pfh_at below (rules Q1-Q8).  Out of scope: PFHRGB. */
#define MVR_PFH_DIM 125             /* 5 * 5 * 5 joint bins (pcl::PFHSignature125) */
#define MVR_PFH_STAGE 256           /* neighbours of one query staged in LDS; above it the tiled path */
typedef struct {
  double radius;        /* setRadiusSearch: finite, > 0, or 0 for k mode                   */
  int    k;             /* setKSearch: 1..MVR_MAX_KNN, or 0 for radius mode; exactly one set */
  int    fma_dist;
} mvr_pfh_params;
int  mvr_cloud_pfh(mvr_ctx *ctx, int slot, const mvr_pfh_params *p,
                   float *pfh,               /* host, n * 125, row = point index; may be NULL  */
                   uint32_t *counts,         /* optional host, n * 125: c_i[h] of rule P5      */
                   uint32_t *neighbor_count  /* optional host, n: n_i of rule P2               */);

/* ---- normals, FPFH and PFH at query points over a search surface (EXTENSION: setSearchSurface / setIndices) ---------------
 * PCL computes descriptors at a few keypoints against the full-resolution scan (setInputCloud(keypoints) with
 * setSearchSurface(scan), or setIndices), and the normals of a downsampled cloud from the scan it came from.  The three
 * entries below are the three above with the query separated from the surface; one query convention serves them.
 *  Q1. Which queries.  indices == NULL: every point of q_slot is a query, rows = n_q, row r answers point r.  Otherwise
 *      rows = n_indices and row r answers point indices[r] of q_slot; indices may be in any order and may repeat.  An index
 *      >= n_q is MVR_E_ARG with nothing written.  rows == 0 is MVR_OK.
 *  Q2. What a query is.  The surface is surface_slot, with that slot's normals (FPFH and PFH need them: F7, P7).  With
 *      q_slot != surface_slot a query is a POSITION only: valid iff its three coordinates are finite; it needs no normal
 *      (PCL: with a search surface set, normals_ belong to the surface).  With q_slot == surface_slot query i IS surface
 *      point i, and F1 / P1 apply to it: a non-finite normal gives a NaN row and count 0.  (Normals need no normal of
 *      anybody: their queries are positions in either case.)
 *  Q3. Neighbourhoods: the library's own rule around the query position -- F2 / P2 radius mode, the f32 d2 with <=, fma_dist;
 *      in k mode (PFH, normals) the mvr_knn(q_slot, surface_slot, k) list of the query, for PFH minus the entries with an
 *      invalid normal.  A surface point at d2 == 0 is a neighbour like any other.
 *  Q4. Values.  Normals: the rules of mvr_cloud_estimate_normals, the covariance relative to the query position, the flip at
 *      the query position, fewer than 3 neighbours NaN.  FPFH: F3-F6; the SPFH of a surface point is its own SPFH in the
 *      surface (F5 of mvr_cloud_fpfh on surface_slot); F6 runs over the query's neighbours, in walk order, in f64; n_i == 0
 *      gives 33 NaN (PCL's "no neighbours"; in the self mode a query is always its own neighbour); an invalid query gives 33
 *      NaN and count 0.  PFH: P3-P6 on the query's neighbourhood; n_i == 0 gives NaN, n_i == 1 zeros; P6's limit holds.
 *  Q5. Equivalence.  A query exactly at surface point i, valid under F1, with the same parameters and the same state of
 *      surface_slot, gets a row BIT-IDENTICAL to row i of the existing call -- signature, counts, neighbor_count, normal and
 *      curvature -- whether it comes through `indices` on the same slot or through a copy of the point in another slot: a
 *      walk's cells and order depend only on the query position and the surface's grid.  PFH counts are in addition
 *      independent of the grid's resolution and of the path taken (P8).
 *  Q6. store_in_slot = 1 (normals) is allowed only with indices == NULL, else MVR_E_ARG; q_slot then gets the normals
 *      (has_normals set) as from mvr_cloud_estimate_normals, the host arrays staying optional.  With store_in_slot = 0
 *      neither slot is modified, the own-coordinates grids of RS10 aside.
 *  Q7. Refusals: everything F7 / P7 list, applied to both slots, the normals requirement to the surface only; all before any
 *      GPU work, with nothing written.  An empty surface with a non-empty query set is MVR_OK with the
 *      empty-neighbourhood rows of Q4.
 *  Q8. Nothing stays on the device after the call.  indices == NULL with q_slot == surface_slot is the existing call (FPFH,
 *      PFH, and normals with store_in_slot = 1; normals with store_in_slot = 0 take the general path, which leaves the slot
 *      alone and gives the same bits).
 * The queries are gathered into an array of positions and sorted by the cell of the surface's grid they fall in (tune key
 * "at_sort" = 0 leaves the sort out; no result depends on it).  FPFH computes the SPFH on demand: a marking walk flags the
 * union of the queries' neighbours, a flagged selection lists them, and only those rows are computed (mvr_ctx_stat
 * "fpfh_at_marked": how many, of the last call).  Out of scope: FPFH in k mode; descriptors kept on the device. */
int  mvr_cloud_estimate_normals_at(mvr_ctx *ctx, int q_slot, const uint32_t *indices, size_t n_indices, int surface_slot,
                                   const mvr_normal_params *p, int store_in_slot,
                                   float *normals   /* optional host, rows * 4: nx ny nz 0 */,
                                   float *curvature /* optional host, rows                 */);
int  mvr_cloud_fpfh_at(mvr_ctx *ctx, int q_slot, const uint32_t *indices, size_t n_indices, int surface_slot,
                       const mvr_fpfh_params *p,
                       float *fpfh              /* host, rows * 33; may be NULL */,
                       uint32_t *neighbor_count /* optional host, rows          */);
int  mvr_cloud_pfh_at(mvr_ctx *ctx, int q_slot, const uint32_t *indices, size_t n_indices, int surface_slot,
                      const mvr_pfh_params *p,
                      float *pfh               /* host, rows * 125; may be NULL */,
                      uint32_t *counts         /* optional host, rows * 125     */,
                      uint32_t *neighbor_count /* optional host, rows           */);

/* ---- SHOT descriptors and their local reference frames (EXTENSION: pcl::SHOTEstimation, SHOT352) -------------------------
 * The 352-float signature of histograms of orientations: 32 volumes (8 azimuth sectors x 2 radial husks x 2 elevation halves)
 * of a repeatable local reference frame, 11 slots of the cosine between the neighbour's normal and the frame's z axis each;
 * linear in the neighbourhood.  PCL was not at hand; the models are pcl/features/impl/shot.hpp (interpolateSingleChannel,
 * normalizeHistogram) and shot_lrf.hpp (getLocalRF), as published; deviations are marked.  A frame is nine f32, row-major:
 * x axis, y axis, z axis.
 * Local reference frame:
 *  L1. A surface point takes part iff its three coordinates are finite; no normal is needed.  A query is a position (Q2); a
 *      non-finite query gets nine NaN and count 0.
 *  L2. Neighbourhood: rule F2 at lrf_radius (0: radius) -- f32 d2 <= (float)(R * R), fma_dist as everywhere -- WITHOUT the
 *      surface points whose three f32 coordinates equal the query's (the query's own point and its exact copies).  FOLLOWING
 *      THE PUBLISHED FILE: getLocalRF skips them (`if (pt.head<3> () == central_point.head<3> ()) continue;`) in the
 *      covariance, in the votes and in the count.  n = the number of the others, which mvr_cloud_shot_lrf reports; n < 5 gives
 *      nine NaN.
 *  L3. All in f64: v_j = (double)p_j - (double)q per component, d_j = sqrt(v_j . v_j), w_j = R - d_j (a weight that a
 *      rounding at the rim makes <= 0 is used as it is, as in PCL), M = sum of w_j v_j v_j^T (six sums), W = sum of w_j.
 *      W == 0 or anything non-finite gives nine NaN.
 *  L4. C = M / W; the cyclic Jacobi of the normals; z0 = the unit eigenvector of the smallest eigenvalue, x0 that of the
 *      largest -- always two different columns of the Jacobi basis, so an isotropic neighbourhood still gets an orthonormal frame.
 *  L5. Sign of a in {x0, z0}: plus = #{j : (v_x a_x + v_y a_y) + v_z a_z >= 0} in f64 over all n neighbours; 2 plus > n keeps
 *      a, 2 plus < n negates it.  DEVIATION on 2 plus == n: PCL looks at five neighbours around the median of FLANN's
 *      distance-sorted list, which a streaming walk does not have; here s = sum of w_j (v_j . a) decides, s < 0 negates.
 *  L6. y = z x x in f64; the nine components are rounded to f32, and the descriptor reads the frame back from those f32: a
 *      frame passed as lrf_in and the frame computed inside the call give the same bits.
 *  L7. Each lane adds in walk order, then a fixed tree: frames are bit-identical from run to run on one grid, and agree across
 *      grid resolutions to rounding.  No floating-point atomics.
 * Descriptor:
 *  H1. The surface needs normals (F7); a surface point contributes iff it is valid under F1.  Query validity is Q2; in the
 *      self mode F1 applies to the query.  An invalid query, or a frame with a NaN (computed or passed in), gives 352 NaN and
 *      count 0 (and, for an invalid query, a NaN frame in lrf_out unless lrf_in was passed, which is returned as it came).
 *  H2. N(i) is rule F2 at radius, the query's own point included; n_i = |N(i)| is what neighbor_count reports.  n_i < 5 gives
 *      352 NaN (THE LIBRARY'S RULE: PCL warns and leaves the row unset).  A neighbour at f64 distance d == 0 adds nothing.
 *  H3. v and d as in L3.  (x, y, z) = (v . X, v . Y, v . Z) in f64, each (a b + c d) + e f, X / Y / Z the f32 frame; a
 *      component with |.| < 1e-30 is set to 0.
 *  H4. Shape: c = n_j . Z in f64, clamped to [-1, 1]; a non-finite c skips the neighbour.  bin = ((1 + c) * 10) / 2,
 *      step = floor(bin + 0.5) in 0..10, t = bin - step.
 *  H5. Volume: vol = 4 s + 2 outer + upper, outer = d > R / 2, upper = z > 0, s the azimuth sector: with a = atan2(y, x),
 *      s = min(7, floor((a + pi) / (pi / 4))), centred on -7 pi / 8 + s pi / 4; x == y == 0 gives s = 0.  The slot of (vol, k)
 *      is 11 vol + k.  (FOLLOWING THE PUBLISHED FILE: s is computed as PCL computes it, from the signs of x and y and the
 *      comparison of |x| with |y| -- the same sector, decided without a libm call, so that no rounding of atan2 moves a
 *      neighbour on a sector border.)
 *  H6. Amounts of one neighbour; home collects, the side amounts go to one neighbouring slot each.
 *      (a) shape: home += 1 - |t|; t > 0: t to (vol, (step + 1) % 10); t < 0: -t to (vol, (step + 9) % 10).  (PCL'S PUBLISHED
 *          QUIRK, kept: the modulus is 10 on 11 slots.)
 *      (b) radial, outer: u = (d - 3R/4) / (R/2); d > 3R/4: home += 1 - u; else home += 1 + u and -u to (vol - 2, step).
 *          Inner: u = (d - R/4) / (R/2); d < R/4: home += 1 + u; else home += 1 - u and u to (vol + 2, step).
 *      (c) elevation, inc = acos(clamp(z / d)).  Lower half (inc > pi/2, or |inc - pi/2| < 1e-30 and z <= 0):
 *          u = (inc - 3pi/4) / (pi/2); inc > 3pi/4: home += 1 - u; else home += 1 + u and -u to (vol + 1, step).  Upper half:
 *          u = (inc - pi/4) / (pi/2); inc < pi/4: home += 1 + u; else home += 1 - u and u to (vol - 1, step).
 *      (d) azimuth, unless x == y == 0: u = (a - centre(s)) / (pi/4) clamped to [-0.5, 0.5]; u > 0: home += 1 - u and u to
 *          ((vol + 4) % 32, step); else home += 1 + u and -u to ((vol + 28) % 32, step).
 *      (e) home goes to (vol, step).
 *      (a) and (d) hand out 1 each; (b) and (c) hand out 1 between the centres of their two halves and 1 - |u| beyond them,
 *      where no slot further out takes the rest: a neighbour adds at most 4 (3 on the z axis), exactly 4 at the centre of a
 *      volume.  (As published the scheme is NOT continuous across a border: home carries the other dimensions' shares with
 *      it from one slot to the next; only the border's own dimension is split half and half.)
 *  H7. Fixed point: every amount w (a negative rounding is clamped to 0) becomes the integer floor(w 2^32 + 0.5) and is added
 *      with an integer atomic into S[352], 64 bits wide: S depends on no order, lane assignment, grid resolution or tune key
 *      (P8's argument).  PCL adds f32 amounts in FLANN's order: a difference of rounding only.
 *  H8. norm = sqrt(sum over ascending b of ((double)S_b)^2); out_b = (float)((double)S_b / norm).  norm == 0 gives 352 NaN
 *      (PCL's 0 / 0; M3 then ignores the row).  `sums` of a NaN row of H1 / H2 are zeros.
 *  H9. Refusals: those of F7 / Q7, plus lrf_radius non-finite or < 0; all before any GPU work, with nothing written.  An
 *      empty cloud is MVR_OK.  All outputs NULL: MVR_OK after the work.  Neither slot is modified, nothing stays on the device.
 * mvr_cloud_shot_lrf needs no normals and reports n of L2.  mvr_cloud_shot_at follows Q1-Q8; Q5 holds for the frames, the sums,
 * the rows and the counts.  One wave per query, three streaming walks (L sums; signs; descriptor), no neighbour list, no cap.
 * Out of scope: colour SHOT (SHOT1344), the k-neighbour mode, descriptors kept on the device. */
#define MVR_SHOT_DIM 352            /* 32 volumes x 11 shape slots (pcl::SHOT352) */
typedef struct {
  double radius;        /* setRadiusSearch: finite, > 0                                   */
  double lrf_radius;    /* setLRFRadius: finite, > 0, or 0 = radius                       */
  int    fma_dist;
} mvr_shot_params;
int  mvr_cloud_shot_lrf(mvr_ctx *ctx, int slot, const mvr_shot_params *p, float *lrf /* host, n * 9 */,
                        uint32_t *neighbor_count /* optional host, n */);
int  mvr_cloud_shot(mvr_ctx *ctx, int slot, const mvr_shot_params *p,
                    const float *lrf_in      /* optional host, n * 9: setInputReferenceFrames */,
                    float *shot              /* host, n * 352; may be NULL                    */,
                    float *lrf_out           /* optional host, n * 9                          */,
                    unsigned long long *sums /* optional host, n * 352: S of rule H7          */,
                    uint32_t *neighbor_count /* optional host, n                              */);
int  mvr_cloud_shot_at(mvr_ctx *ctx, int q_slot, const uint32_t *indices, size_t n_indices, int surface_slot,
                       const mvr_shot_params *p, const float *lrf_in /* optional host, rows * 9 */, float *shot, float *lrf_out,
                       unsigned long long *sums, uint32_t *neighbor_count);

/* ---- feature matching and coarse alignment (EXTENSION: pcl::SampleConsensusPrerejective) -------------------------------
 * What brings a scan without a pose prior within the capture range of mvr_icp_align.  The reference pins no PCL version and
 * PCL was not at hand: the models are pcl/registration/impl/sample_consensus_prerejective.hpp,
 * correspondence_rejection_poly.hpp (thresholdPolygon) and pcl::KdTreeFLANN<FPFHSignature33> with flann::L2_Simple<float>, as
 * published; deviations are marked.
 *
 * mvr_feature_knn: exact k nearest neighbours in feature space.  q / t: host arrays, row = point, `dim` floats per row.
 * dim must be 33 (3 * MVR_FPFH_BINS), 125 (MVR_PFH_DIM) or 352 (MVR_SHOT_DIM), 1 <= k <= MVR_MAX_KNN, else MVR_E_ARG
 * before any GPU work.  idx / d2: host, nq * k, row-major (either may be NULL).
 *  M1. Distance, FLANN's L2_Simple: acc = 0; for b = 0..dim - 1 { diff = q[b] - t[b]; acc = acc + diff * diff; } -- all f32,
 *      every operation rounded, in this order, never contracted.  There is no fma variant.
 *  M2. Order: the k smallest under the key (d2 bits, index), ascending; ties go to the lower index -- the key of mvr_knn.
 *  M3. Non-finite rows: a target row with a non-finite component is never listed, and neither is a pair whose d2 is not
 *      finite; a non-finite query row gets UINT32_MAX / +inf in all k entries, and so does the tail of a list beyond the
 *      listable targets (rules N1-N3 carried over).
 *  The target is split over blocks as well as the queries (tune key "feat_split", 0 = by the launch size); the partial
 *  lists are merged under the same total order, so the result does not depend on the split.
 *
 * mvr_pose_scores: inliers and error of `count` poses of src_slot against tgt_slot in one call.  T: count * 16 floats, each
 * a column-major 4 x 4.  inliers / error: host, `count` entries (either may be NULL).
 *  S1. For pose h and source point i: p' = mvr_cloud_transform_f32's arithmetic on p_i; its exact nearest target point under
 *      the library's f32 distance (fma_dist as everywhere); i is an inlier iff (double)d2 < max_dist * max_dist -- strictly, as
 *      in PCL's getFitness.  A non-finite p', a non-finite target point and an empty target give no inlier.
 *  S2. inliers[h] is the exact count; error[h] = (sum of the inliers' (double)d2) / count, DBL_MAX when the count is 0.  The
 *      sum is f64 in a fixed order: one partial per block of 256 source points in the source's grid order (a fixed tree inside
 *      the block), the partials added in ascending order.  No tune key changes it ("score_chunk": poses per launch).
 *  Neither slot is modified and no posed copy is materialised.  MVR_E_ARG for a NULL ctx, a bad slot, a NULL T with count > 0,
 *  or a max_dist that is not finite and > 0.
 *
 * mvr_align_prerejective: pcl::SampleConsensusPrerejective::computeTransformation.  src_feat / tgt_feat: host, 33 floats per
 * point of the slot.  DEVIATION: PCL draws with rand(); this is a pure function of its arguments (seed included), bit for bit.
 *  A1. Eligible source points: finite coordinates and 33 finite features, in ascending index; ne of them.  ne < nr_samples:
 *      MVR_OK with converged = 0 and nothing scored (every traced iteration has status 2).
 *  A2. Draws, arithmetic mod 2^64, G = 0x9E3779B97F4A7C15:  mix(x): z = x; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
 *      z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31.   draw(i, j, m) = ((mix(seed + G * (16 i + j + 1)) >> 32) * m) >> 32.
 *      Sample j of iteration i: r = draw(i, j, ne - j); for every earlier sample POSITION c of this iteration, in ascending
 *      order of c: if (r >= c) ++r -- distinct samples without rejection; the source point is eligible[r].
 *  A3. Matches: the table of rule M, k entries, from the eligible source rows into tgt_feat.  kk = the non-empty entries of
 *      sample j's list; the match is entry draw(i, 8 + j, kk).  kk = 0 for any sample: status 2 (its tgt entry UINT32_MAX).
 *  A4. Polygon (thresholdPolygon) over the edges (j, (j + 1) % nr_samples): ds / dt = the library's f32 d2 between the two
 *      source points / the two matches (fma_dist); sim = ds < dt ? ds / dt : dt / ds in f32; the edge passes iff
 *      sim >= (float)(similarity * similarity) (a NaN, 0 / 0 included, fails).  A failing edge: status 0, counted in `rejected`.
 *  A5. Pose: the estimator of mvr_icp_align -- f64 means and covariance of the nr_samples pairs in sample order, the host
 *      SVD (Eigen::umeyama without scaling), cast to f32.
 *  A6. Score: rule S over ALL points of the source slot; fraction = inliers / (double)n_src (the slot's size, as PCL).  A
 *      pose is taken iff fraction >= inlier_fraction && error < lowest, poses visited in iteration order, lowest = DBL_MAX
 *      at the start.  A non-NULL guess is scored first by the same test and recorded as best_iteration = -1.
 *  Result: converged = a pose was taken; T = that pose (none: the guess, else the identity, with inliers = 0 and
 *  error = DBL_MAX, best_iteration = -1); rejected / scored = iterations with status 0 / 1.  trace (optional, max_iterations
 *  entries): per iteration its status, samples, matches and -- status 1 -- inliers, error and T (otherwise zeros).
 *  MVR_E_ARG, before any GPU work, for a NULL ctx / params / result / feature table, a bad slot, max_iterations < 0,
 *  nr_samples outside 3..8, k outside 1..MVR_MAX_KNN, similarity outside [0, 1), max_dist not finite and > 0, or
 *  inlier_fraction outside (0, 1].  The draws, matches and polygon tests of all iterations are one launch; the surviving poses
 *  are solved on the host and scored through the kernel of mvr_pose_scores.
 * mvr_align_prerejective_dim: the same with `dim` floats per row of the two feature tables, dim = 33, 125 or 352 (else MVR_E_ARG):
 * rules A1-A6 with "33" read as dim.  mvr_align_prerejective is this with dim = 33.
 * Out of scope: SampleConsensusInitialAlignment, descriptors of lengths other than 33, 125 and 352; MFMA and the unit-norm
 * shortcut 2 - 2 q.t for SHOT rows (M1's sum is kept term by term at every length).
 * (CorrespondenceRejectorSampleConsensus over the matches of mvr_feature_knn is mvr_reject_sample_consensus, rules C1-C12.) */
int  mvr_feature_knn(mvr_ctx *ctx, const float *q, size_t nq, const float *t, size_t nt, int dim, int k,
                     uint32_t *idx /* nq * k */, float *d2 /* nq * k */);
int  mvr_pose_scores(mvr_ctx *ctx, int src_slot, int tgt_slot, const float *T /* count * 16, column-major */, size_t count,
                     double max_dist, int fma_dist, uint32_t *inliers /* count */, double *error /* count */);
#define MVR_PREREJ_MAX_SAMPLES 8
typedef struct {
  int      max_iterations;   /* setMaximumIterations: >= 0                                  */
  int      nr_samples;       /* setNumberOfSamples: 3..8                                    */
  int      k;                /* setCorrespondenceRandomness: 1..MVR_MAX_KNN                 */
  double   similarity;       /* setSimilarityThreshold: [0, 1)                              */
  double   max_dist;         /* setMaxCorrespondenceDistance: finite, > 0                   */
  double   inlier_fraction;  /* setInlierFraction: (0, 1]                                   */
  uint64_t seed;             /* ours: PCL draws with rand()                                 */
  int      fma_dist;
} mvr_prerej_params;
typedef struct {
  int      converged;
  int      best_iteration;   /* -1: the guess (or, without converged, nothing)              */
  uint32_t inliers;
  double   error;
  uint32_t rejected, scored;
  float    T[16];
} mvr_prerej_result;
typedef struct {
  int      status;           /* 0 polygon-rejected, 1 scored, 2 no match                    */
  uint32_t src[MVR_PREREJ_MAX_SAMPLES], tgt[MVR_PREREJ_MAX_SAMPLES], inliers;
  double   error;
  float    T[16];
} mvr_prerej_trace;
int  mvr_align_prerejective(mvr_ctx *ctx, int src_slot, int tgt_slot, const float *src_feat, const float *tgt_feat,
                            const mvr_prerej_params *params, const float *guess /* optional, 16 */,
                            mvr_prerej_result *result, mvr_prerej_trace *trace /* optional, max_iterations */);
int  mvr_align_prerejective_dim(mvr_ctx *ctx, int src_slot, int tgt_slot, const float *src_feat, const float *tgt_feat, int dim,
                                const mvr_prerej_params *params, const float *guess /* optional, 16 */,
                                mvr_prerej_result *result, mvr_prerej_trace *trace /* optional, max_iterations */);

/* ---- intrinsic shape signature keypoints (EXTENSION: pcl::ISSKeypoint3D) -----------------------------------------------
 * What chooses the points that carry a descriptor into the matcher: a row of a feature table that is overwritten with NaN is
 * ineligible as a sample (A1) and never listed as a match (M3), so a non-keypoint is a NaN row.  The reference pins no PCL
 * version and PCL was not at hand; the model is pcl/keypoints/impl/iss_3d.hpp (getScatterMatrix, getBoundaryPoints,
 * detectKeypoints), as published; deviations are marked.  K1-K8 are the detector with border_radius == 0
 * (mvr_cloud_iss_keypoints); K9-K11 add the border handling (mvr_cloud_iss_keypoints_border).
 *  K1. A point is VALID when its three coordinates are finite.  An invalid point is nobody's neighbour and never a keypoint;
 *      its saliency is 0 and both its counts are 0; no query walks the grid because of one (rules N2 and N5 above).
 *  K2. Neighbourhood of radius r: every valid j with d2(i, j) <= (float)(r * r) under the f32 distance of mvr_nn / mvr_knn,
 *      i itself included -- exactly the radius mode of mvr_cloud_estimate_normals; fma_dist = 1 selects the fma chain.
 *  K3. Scatter: the sum over the neighbourhood of salient_radius of (p_j - p_i)(p_j - p_i)^T in f64, in walk order; the
 *      differences are taken in f64 from the f32 coordinates; the sum is NOT divided by the count (as PCL).  salient_count[i]
 *      is the size of that neighbourhood; below min_neighbors the saliency is 0.  (PCL accumulates the f32 differences
 *      into a double matrix.)
 *  K4. Eigenvalues e1 >= e2 >= e3 of the scatter by the library's cyclic Jacobi in f64 (PCL: Eigen's SelfAdjointEigenSolver).
 *      Point i is SALIENT iff all of: the three are finite, e3 >= 0, e2 / e1 < gamma_21, e3 / e2 < gamma_32, e3 > 0.  The
 *      divisions are IEEE: a NaN ratio fails.  saliency[i] = e3 for a salient point, else 0.
 *  K5. Non-maximum suppression: a salient i is a keypoint iff nms_count[i] >= min_neighbors, with nms_count[i] the size of
 *      its neighbourhood of non_max_radius, and no j of that neighbourhood has saliency[i] < saliency[j].  The comparison is
 *      strict: equal saliencies are both kept, as in PCL.  nms_count is 0 for a point that is not salient.
 *  K6. Output: the keypoints go to dst_slot in ascending original index, w = 1; the source's normals follow their points, as
 *      in the outlier filters.  The output is a NEW point set: orderings, grids and pose bookkeeping are dropped.  dst_slot
 *      may equal src_slot.  dst_slot == -1 fills the host arrays only and leaves every slot untouched.  kept_index (optional,
 *      host, capacity = source size) receives the keypoints' original indices, ascending; n_out (optional) their number;
 *      saliency / salient_count / nms_count (optional, host) one entry per SOURCE point.
 *  K7. MVR_E_ARG, before any GPU work and with nothing written, for a NULL ctx / params, a bad slot, a radius that is
 *      non-finite or <= 0, a non-finite gamma, min_neighbors < 0, a cloud above 0x7FFFFFF0 points, or a cloud whose points are
 *      stale because a pipelined run is in flight.  An empty cloud is MVR_OK with an empty output.
 *  K8. Bit-identical from run to run on one grid: one thread per query, sums in walk order, no floating-point atomics.
 *  K9. mvr_cloud_iss_keypoints_border with border parameters whose border_radius > 0 (setBorderRadius; angle_threshold is
 *      setAngleThreshold): the source slot must have normals, else MVR_E_ARG.  edge[i] = rule B of mvr_cloud_boundary at
 *      border_radius with the caller's angle_threshold, this call's min_neighbors and fma_dist.  On top of K7, MVR_E_ARG for
 *      a border_radius that is non-finite or < 0 and for an angle_threshold outside B6's range.
 *  K10. border[i] = i is valid and some j of its neighbourhood of border_radius (K2; i included) has edge[j].
 *  K11. A border point has saliency 0, salient_count 0 and nms_count 0 and is never a keypoint; everything else of K3-K6 is
 *      unchanged.  A border point therefore never suppresses a neighbour.  (PCL skips the border points before the saliency
 *      test in the same way.)  edge / border (optional, host) receive one byte per SOURCE point.
 *  With NULL border parameters, or border_radius == 0 (the threshold is then not looked at), every result equals
 *  mvr_cloud_iss_keypoints bit for bit -- that entry IS this call with NULL -- and edge / border are all 0.
 * Out of scope: setSearchSurface, estimating the normals inside the call (setNormalRadius: pcl::ISSKeypoint3D of
 * mvr/registration.hpp does it with mvr_cloud_estimate_normals first), and the other keypoint detectors (Harris3D, SIFT,
 * NARF, ...). */
typedef struct {
  double salient_radius;     /* setSalientRadius: finite, > 0 */
  double non_max_radius;     /* setNonMaxRadius:  finite, > 0 */
  double gamma_21, gamma_32; /* setThreshold21 / setThreshold32 (PCL default 0.975 each): finite */
  int    min_neighbors;      /* setMinNeighbors (PCL default 5): >= 0 */
  int    fma_dist;
} mvr_iss_params;
int  mvr_cloud_iss_keypoints(mvr_ctx *ctx, int dst_slot /* -1: none */, int src_slot, const mvr_iss_params *p,
                             size_t *n_out, uint32_t *kept_index, double *saliency /* n */,
                             uint32_t *salient_count /* n */, uint32_t *nms_count /* n */);
typedef struct {
  double border_radius;      /* setBorderRadius: finite, >= 0; 0: no border */
  double angle_threshold;    /* setAngleThreshold (PCL default pi / 2): B6's range */
} mvr_iss_border_params;
int  mvr_cloud_iss_keypoints_border(mvr_ctx *ctx, int dst_slot /* -1: none */, int src_slot, const mvr_iss_params *p,
                             const mvr_iss_border_params *border_params /* NULL or radius 0: none */, size_t *n_out,
                             uint32_t *kept_index, double *saliency /* n */, uint32_t *salient_count /* n */,
                             uint32_t *nms_count /* n */, uint8_t *edge /* n, optional */, uint8_t *border /* n, optional */);

/* ---- boundary points (EXTENSION: pcl::BoundaryEstimation) --------------------------------------------------------------
 * Which points of a partial surface lie on its rim: the neighbours of a point are projected onto its tangent plane and the
 * point is a boundary point when they leave an angular gap wider than a threshold.  PCL was not at hand; the model is
 * pcl/features/impl/boundary.hpp (isBoundaryPoint, getCoordinateSystemOnPlane, computeFeature), as published, in radius mode
 * with the cloud its own search surface; deviations are marked.
 *  B1. Valid points and neighbourhoods are those of K1 and K2 above: the f32 distance with d2 <= (float)(radius * radius), i
 *      itself included, fma_dist = 1 the fma chain.  neighbor_count[i] = the size of that neighbourhood, 0 for an invalid
 *      point.  The cloud is its own search surface.
 *  B2. Tangent basis from the point's normal n (f32, the slot's): Eigen's generic unitOrthogonal, then u = n x v.
 *      maxi = the first index of the largest |n_c|; sndi = (maxi == 0) ? 1 : 0;
 *      inv = 1.0f / sqrtf(n[sndi] * n[sndi] + n[maxi] * n[maxi]); v[maxi] = -n[sndi] * inv, v[sndi] = n[maxi] * inv, the third
 *      component 0; u = (n.y v.z - n.z v.y, n.z v.x - n.x v.z, n.x v.y - n.y v.x), every operation rounded to f32, never
 *      contracted.  The normal is taken as it is: it is not normalised, and its sign does not change any result.
 *      DEVIATION: a normal with a non-finite component, or one for which a component of u or v comes out non-finite (the zero
 *      normal), makes the point NOT a boundary point with max_gap = 0; its neighbor_count is still B1's.  (PCL sorts NaNs.)
 *  B3. An angle for every neighbour j, in walk order: d = p_j - p_i in f32; j is skipped when all three differences are
 *      exactly 0 (i itself and its exact copies); otherwise a_j = atan2f(v.x d.x + v.y d.y + v.z d.z, u.x d.x + u.y d.y +
 *      u.z d.z), the sums left to right in f32.
 *  B4. max_dif = the largest, in f32 and starting from FLT_MIN, of the differences of consecutive angles in ascending order
 *      and of the wrap-around (2 * (float)M_PI - a_last) + a_first.
 *  B5. Point i is a boundary point iff all of: i is valid; neighbor_count[i] >= 3; neighbor_count[i] >= min_neighbors; at least
 *      one angle was taken; max_dif > (float)angle_threshold, strictly.  min_neighbors = 0 is
 *      pcl::BoundaryEstimation::computeFeature; the ISS detector passes its own (K9).
 *      max_gap (optional): the angles are not sorted.  The circle is cut into 16 equal sectors, sector(a) = floor((a + pi)
 *      * 16 / 2 pi) in f32, clamped to 0..15; max_gap[i] is the largest, from FLT_MIN, of (smallest angle of the next occupied
 *      sector - largest angle of this one) over the occupied sectors in ascending order and of the wrap-around of B4 from the
 *      last maximum and the first minimum.  Those are the differences of B4 that lie between two sectors, from the same f32
 *      operands; two angles of one sector are less than a sector width (pi / 8) apart.  So max_gap[i] == max_dif whenever
 *      max_dif is at least a sector width, and is below a sector width otherwise; with angle_threshold >= two sector widths
 *      (B6) the test of B5 on max_gap IS the test on max_dif.  max_gap[i] = 0 for an invalid point, under B2's deviation, and
 *      when no angle was taken.
 *  B6. MVR_E_ARG, before any GPU work and with nothing written, for a NULL ctx / params, a bad slot, a slot without normals,
 *      a radius that is non-finite or <= 0, min_neighbors < 0, an angle_threshold outside [MVR_BOUNDARY_MIN_ANGLE, 2 pi) (a
 *      non-finite one included), a cloud above 0x7FFFFFF0 points, or a cloud whose points are stale because a pipelined run
 *      is in flight.  An empty cloud is MVR_OK.  All three outputs NULL: MVR_OK after the work.
 *  B7. The slot is not modified.  Bit-identical from run to run on one grid: one thread per query, minima and maxima only.
 * Out of scope: the k-neighbour mode (setKSearch), setSearchSurface / setIndices, the organized-cloud border extractors. */
#define MVR_BOUNDARY_MIN_ANGLE 0.78539816339744830962 /* pi / 4: two of the 16 sectors */
typedef struct {
  double radius;             /* setRadiusSearch: finite, > 0 */
  double angle_threshold;    /* setAngleThreshold (PCL default pi / 2): [MVR_BOUNDARY_MIN_ANGLE, 2 pi) */
  int    min_neighbors;      /* >= 0; 0: pcl::BoundaryEstimation */
  int    fma_dist;
} mvr_boundary_params;
int  mvr_cloud_boundary(mvr_ctx *ctx, int slot, const mvr_boundary_params *p, uint8_t *boundary /* n */,
                        float *max_gap /* n, optional */, uint32_t *neighbor_count /* n, optional */);

/* ---- plane segmentation (EXTENSION: pcl::SACSegmentation with SAC_RANSAC, pcl::ExtractIndices) ---------------------------
 * Takes the largest plane -- the platter or the table a scanned object stands on -- out of a cloud.  PCL was not at hand; the
 * model is pcl/sample_consensus/impl/ransac.hpp, sac_model_plane.hpp, sac_model_perpendicular_plane.hpp,
 * pcl/segmentation/impl/sac_segmentation.hpp and pcl/filters/impl/extract_indices.hpp, as published; deviations are marked.
 * Every f32 operation below is rounded on its own and never contracted (the build has -ffp-contract=off).
 *  P1. Valid points: a point is VALID when its three coordinates are finite; nv = their number.  An invalid point is never
 *      sampled and never an inlier.  nv < 3: MVR_OK with found = 0 and no attempt made.
 *  P2. Draws: mix / draw of rule A2, unchanged.  Sample j (0..2) of ATTEMPT t: r = draw(t, j, nv - j); then, for the earlier
 *      samples of this attempt TAKEN IN ASCENDING ORDER OF THEIR VALUE r (not in the order they were drawn): if (r >= that) ++r.
 *      The point is the r-th valid point in ascending original index.  The three are distinct by construction.
 *      DEVIATION: PCL draws with rand() and has an isSampleGood retry loop; there is none here.
 *  P3. Model from the samples p0, p1, p2, in f32: e1 = p1 - p0, e2 = p2 - p0; n = (e1.y e2.z - e1.z e2.y, e1.z e2.x - e1.x e2.z,
 *      e1.x e2.y - e1.y e2.x); len2 = (n.x n.x + n.y n.y) + n.z n.z; len = sqrtf(len2); (a, b, c) = n / len, a division per
 *      component; d = -((a p0.x + b p0.y) + c p0.z).  The attempt is SKIPPED (status 0; its traced coefficients and count are 0)
 *      when len2 is not > 0 or any of a, b, c, d is non-finite.  DEVIATION: PCL tests collinearity by a ratio of differences.
 *  P4. SACMODEL_PERPENDICULAR_PLANE (model 1): cs = |(a A.x + b A.y) + c A.z| / (sqrt((a a + b b) + c c) * sqrt((A.x A.x +
 *      A.y A.y) + A.z A.z)) in f64 from the f32 normal and the caller's axis A, the second root taken once on the host.  The
 *      model is INVALID (status 3) iff cs < cos(eps_angle), the cosine taken once on the host.  An invalid model is a COUNTED
 *      attempt with 0 inliers, as in PCL, whose countWithinDistance returns 0 for it.
 *  P5. Distance of a point (x, y, z) in f32: t = a x; t = t + b y; t = t + c z; t = t + d; with fma_dist the two middle steps
 *      are t = fmaf(b, y, t) and t = fmaf(c, z, t).  The point is an inlier iff (double)fabsf(t) < threshold, strictly (the
 *      kernels compare with the smallest f32 that is >= threshold, which is the same test).  An invalid point gives a
 *      non-finite t and is never an inlier.
 *  P6. The count of an attempt is the exact integer number of inliers: independent of order and of launch shape.
 *  P7. The loop is PCL's, replayed on the host over the attempts t = 0, 1, ... in order:
 *        iterations = 0, skipped = 0, k = 1, best_count = -1;
 *        while (iterations < k && skipped < 10 * max_iterations) {
 *          attempt t; if it is skipped { ++skipped; continue; }
 *          if (count > best_count) {                 -- strictly: the first of equal counts stays
 *            best_count = count; best = t; w = best_count / (double)nv;      DEVIATION: PCL divides by all indices
 *            pno = 1 - w * w * w, clamped to [DBL_EPSILON, 1 - DBL_EPSILON]; k = log(1 - probability) / log(pno); }
 *          ++iterations; if (iterations > max_iterations) break; }
 *      The break is PCL's own off-by-one -- up to max_iterations + 1 counted attempts -- and is kept.  `attempts` = the attempts
 *      made (iterations + skipped).  found = (best_count > 0): some counted attempt had an inlier.  Under model 0 a counted
 *      attempt has its own three samples within any sensible threshold, so there found means "an attempt was counted";
 *      under model 1 every attempt may be invalid.  (PCL would keep a model without inliers and SACSegmentation would return
 *      empty indices: here that is found = 0.)  best_attempt = best when found, else -1.
 *  P8. Attempts are generated and scored in chunks (tune key "sac_chunk": 1..256 attempts per chunk; 0, default: chosen by the
 *      library); the attempts of a chunk beyond the point where the loop stops are discarded.  Result and trace are
 *      bit-identical for every chunk size.
 *  P9. The inliers are those of P5 under the best attempt's coefficients: ransac_coefficients and ransac_inliers.
 *  P10. optimize (setOptimizeCoefficients): with q = the first sample of the best attempt, the sums of dx, dy, dz, dx dx,
 *      dx dy, dx dz, dy dy, dy dz, dz dz over the inliers, (dx, dy, dz) = (double)p - (double)q, in f64 in a fixed order as in
 *      rule S2: one partial per block of 256 consecutive ORIGINAL indices (a point that is no inlier adds +0), the fixed tree
 *      v[i] += v[i + s] for s = 128, 64, ..., 1 inside a block, the partials added in ascending order.  Mean and covariance
 *      from them as the normals do (inv = 1 / count; m = sum * inv; C.xy = xy * inv - m.x * m.y); the eigenvector of the
 *      smallest eigenvalue by the library's cyclic Jacobi, normalised; turned so that its dot product with the RANSAC normal
 *      is >= 0 (DEVIATION: PCL leaves the sign to Eigen); d = -((n.x M.x + n.y M.y) + n.z M.z) with M = q + m, all in f64;
 *      then the four are cast to f32.  The inliers are selected again (P5) with the refined coefficients, as
 *      SACSegmentation::segment does.  With fewer than 3 inliers, or a non-finite refined coefficient, the RANSAC
 *      coefficients and inliers stay.  `coefficients` and `inliers` are the final ones either way.
 *  P11. Output: inlier_index (optional, host, capacity = source size) = the inliers' original indices, ascending;
 *      inlier_flag (optional, host) = one byte per SOURCE point.  dst_slot receives the inliers, or with `negative` every
 *      other point of the source, invalid points included, as ExtractIndices::setNegative does; in ascending original index,
 *      normals following their points; a NEW point set as in K6; dst_slot may equal src_slot; dst_slot == -1 leaves every slot
 *      untouched.  *n_out (optional) = the number of points of that output set.  found = 0: no inliers, so the output is
 *      empty, or with `negative` a copy of the source.  trace[t] (optional) for every attempt made, t < trace_cap: status
 *      (0 skipped, 1 counted, 3 invalid under P4), the samples' original indices, the coefficients, the count (0 unless
 *      status 1) and k after the attempt.
 *  P12. MVR_E_ARG, before any GPU work and with nothing written, for a NULL ctx / params / result, a bad slot, dst_slot < -1,
 *      a model outside 0..1, a threshold that is non-finite or <= 0, max_iterations < 1 or above 1 << 24, a probability
 *      outside (0, 1), under model 1 an axis with a non-finite component or all zero or an eps_angle outside (0, pi / 2], a
 *      cloud above 0x7FFFFFF0 points, or a cloud whose points are stale because a pipelined run is in flight.  An empty cloud
 *      is MVR_OK with found = 0.  Bit-identical from run to run: integer atomics only, every f64 sum in the order of P10.
 * Out of scope: other models (sphere, cylinder, line, normal plane), other estimators (LMedS, MSAC, PROSAC),
 * setSamplesMaxDist, setIndices on the segmentation. */
typedef struct {
  int      model;            /* 0: SACMODEL_PLANE, 1: SACMODEL_PERPENDICULAR_PLANE */
  double   threshold;        /* setDistanceThreshold: finite, > 0 */
  int      max_iterations;   /* setMaxIterations: >= 1 */
  double   probability;      /* setProbability: in (0, 1) */
  int      optimize;         /* setOptimizeCoefficients */
  double   axis[3];          /* setAxis (model 1): finite, not all zero */
  double   eps_angle;        /* setEpsAngle (model 1): in (0, pi/2] */
  uint64_t seed;             /* ours: PCL draws with rand() */
  int      negative;         /* ExtractIndices::setNegative, for dst_slot */
  int      fma_dist;
} mvr_sac_params;
typedef struct { int found; uint32_t inliers, ransac_inliers; int iterations, attempts, skipped, best_attempt;
                 double k; float coefficients[4], ransac_coefficients[4]; } mvr_sac_result;
typedef struct { int status; uint32_t sample[3]; float coefficients[4]; uint32_t inliers; double k; } mvr_sac_trace;
int  mvr_cloud_segment_plane(mvr_ctx *ctx, int dst_slot /* -1: none */, int src_slot, const mvr_sac_params *p,
                             mvr_sac_result *result, size_t *n_out, uint32_t *inlier_index /* cap = source size */,
                             uint8_t *inlier_flag /* n, optional */, mvr_sac_trace *trace /* optional */, size_t trace_cap);
/* pcl::ExtractIndices::filter: dst_slot (may be src_slot) receives the points of src_slot whose index is listed in `index`
 * (host, count entries, each below the source size, in any order, repeats allowed -- a point is taken once), or with
 * `negative` all the others; ascending original index, normals following, a new point set (P11's tail).  MVR_E_ARG for a NULL
 * ctx, a bad slot, a NULL index with count > 0, an index out of range, or a stale or oversized cloud. */
int  mvr_cloud_extract_indices(mvr_ctx *ctx, int dst_slot, int src_slot, const uint32_t *index, size_t count, int negative,
                               size_t *n_out);

/* ---- Euclidean cluster extraction (EXTENSION: pcl::EuclideanClusterExtraction, pcl::extractEuclideanClusters with normals) --
 * What is left of a scan once the platter is out (mvr_cloud_segment_plane) is the object plus whatever stood beside it; this
 * call reports the clusters of a cloud, largest first, and can keep the first few.  PCL was not at hand; the model is
 * pcl/segmentation/impl/extract_clusters.hpp and extract_clusters.h, as published; where PCL differs the rule here is the
 * library's and the deviation is marked.  One thread per point walks the cloud's own grid (the walks of rules N, B and K) and
 * unites linked points in a lock-free union-find; see csrc/mvr_cluster.hip.
 *  E1. Active points: with index == NULL every point is active, whatever `negative` says.  Otherwise the listed points are
 *      active (host, index_count entries, any order, repeats allowed, each below the source size; index_count may be 0), or
 *      with `negative` all the others.  An inactive point links to nothing and is reported nowhere; its label is UINT32_MAX.
 *  E2. Link: two active points with finite coordinates link iff d2 <= (float)(tolerance * tolerance), d2 the library's f32
 *      distance ((dx dx + dy dy) + dz dz, every operation rounded; with fma_dist the fma chain, as everywhere).  The same
 *      ball as B1 and K2.  DEVIATION: FLANN's radius search is strict (d2 < r2).
 *  E3. With use_normals the link also needs dot > cos(eps_angle), dot = ((double)a.x * b.x + (double)a.y * b.y) +
 *      (double)a.z * b.z from the slot's f32 normals, every f64 operation rounded on its own, the cosine taken once on the
 *      host.  This is PCL's fabs(acos(dot)) < eps_angle: opposite normals do not link, even under eps_angle = pi.  DEVIATION: a
 *      dot that rounding pushed above 1 links here (PCL's acos gives NaN there, which fails its test).  A NaN dot links
 *      nothing.  The rule is symmetric in the pair, so the clusters are the connected components of the link graph; PCL's
 *      flood fill finds the same components (a point may be reached through any chain of links).
 *  E4. A point with a non-finite x, y or z links to nothing and is a component of one point (as D1, D2); it takes no part in
 *      sizing the grid.  A cloud with no finite point gives components of size 1 and MVR_OK.
 *  E5. A component is a cluster iff max(min_size, 1) <= size <= max_size.  too_small counts the components below
 *      max(min_size, 1), too_large those of the others above max_size.  min_size > max_size gives no cluster and MVR_OK.
 *  E6. Order: clusters by size descending (PCL's order), equal sizes by their smallest member index ascending (PCL's
 *      std::sort leaves that open); the members of a cluster in ascending index (as PCL sorts them).
 *  E7. Outputs (host, each optional): cluster_index = the concatenated member lists, n_clustered entries (capacity: the
 *      source size); cluster_offset[c] and cluster_offset[c + 1] bound cluster c in it -- only the first m = min(n_clusters,
 *      offset_cap - 1) clusters get offsets (m + 1 entries written, none with offset_cap = 0), result->n_clusters is always
 *      the full number, so a caller sees a truncation; label[i] (one per source point) = the rank of point i's cluster, else
 *      UINT32_MAX.  result: n_active (E1), n_components (of the active points), n_clusters, n_clustered (points in
 *      clusters), largest (size of cluster 0; 0 without one), too_small, too_large.  dst_slot receives the union of the first
 *      min(keep, n_clusters) clusters in ascending original index, normals following, a NEW point set as in P11's tail; it
 *      may equal src_slot; dst_slot == -1 touches no slot.  *n_out (optional) = the points dst_slot received (0 without one).
 *  E8. MVR_E_ARG, before any GPU work and with nothing written, for a NULL ctx / params / result, a bad slot, dst_slot < -1,
 *      a tolerance that is non-finite or <= 0, keep == 0 with dst_slot >= 0, use_normals on a slot without normals or with
 *      an eps_angle outside (0, pi], a NULL index with index_count > 0, an index out of range, a cloud above 0x7FFFFFF0
 *      points, or a cloud whose points are stale because a pipelined run is in flight.  An empty cloud is MVR_OK with zeros.
 *      Bit-identical from run to run and for every grid resolution: integer atomics only, and the root of a component is its
 *      smallest member whatever the order of the unions.
 * Out of scope: pcl::ConditionalEuclideanClustering, region growing, labelled (per-label) clustering. */
typedef struct {
  double   tolerance;     /* setClusterTolerance: finite, > 0 */
  uint32_t min_size;      /* setMinClusterSize (0 is 1) */
  uint32_t max_size;      /* setMaxClusterSize */
  int      use_normals;   /* extractEuclideanClusters(cloud, normals, ...) */
  double   eps_angle;     /* with use_normals: in (0, pi] */
  int      negative;      /* how `index` is read, as in mvr_cloud_extract_indices */
  uint32_t keep;          /* dst_slot: the first `keep` clusters (>= 1) */
  int      fma_dist;
} mvr_cluster_params;
typedef struct { uint32_t n_active, n_components, n_clusters, n_clustered, largest, too_small, too_large; } mvr_cluster_result;
void mvr_cluster_default_params(mvr_cluster_params *p);   /* PCL's: min 1, max INT32_MAX, no normals, keep 1; tolerance 0 (to be set) */
int  mvr_cloud_euclidean_clusters(mvr_ctx *ctx, int dst_slot /* -1: none */, int src_slot, const mvr_cluster_params *p,
                                  const uint32_t *index, size_t index_count,      /* setIndices; NULL: every point */
                                  mvr_cluster_result *result, size_t *n_out,
                                  uint32_t *cluster_offset, size_t offset_cap,    /* optional */
                                  uint32_t *cluster_index /* cap = source size, optional */,
                                  uint32_t *label /* one per source point, optional */);

/* CorrespondenceEstimation::determineReciprocalCorrespondences(corrs, max_d)
 * (registrator.cpp:496-502, 644-649); reciprocal = 0 gives
 * determineCorrespondences.  Outputs are host arrays of capacity `cap`
 * (pcl::Correspondence fields index_query / index_match / distance(squared)),
 * in ascending query order.  *m = number found (may exceed cap: truncated). */
int  mvr_correspondences(mvr_ctx *ctx, int src_slot, int tgt_slot, double max_dist,
                         int reciprocal, int fma_dist,
                         int32_t *query, int32_t *match, float *dist2, size_t cap, size_t *m);

/* correspondences + TransformationEstimationSVD accumulation (K2,K3,K5,K6) of
 * one scan pair; the correspondences stay on the device.  This is the
 * shardable per-pair unit of the ring/global mode (registrator.cpp:482-502,
 * 640-651).  q_begin/q_count restrict the SOURCE queries to a sub-range (for
 * splitting one pair over ranks; sums are then partial: n, n*mean, n*mse and
 * raw second moments add across sub-ranges) -- pass 0, SIZE_MAX for all.
 * A sub-range is a range of the walk's POSITIONS: source indices q_begin ..
 * q_begin + q_count - 1 under the brute-force search; under the culled search
 * the points at those positions of the context's ordering of the source
 * (mvr_debug_order: position -> index).  Either way the sub-ranges of a split
 * of 0 .. n - 1 cover every source point once, which is all a split needs. */
int  mvr_pair_moments(mvr_ctx *ctx, int src_slot, int tgt_slot, double max_dist,
                      int reciprocal, int fma_dist, mvr_pair_moments_t *out);
int  mvr_pair_moments2(mvr_ctx *ctx, int src_slot, int tgt_slot, double max_dist,
                       int reciprocal, int fma_dist, size_t q_begin, size_t q_count,
                       const double origin[3], mvr_pair_moments2_t *out);
/* device-output variant: writes 32 doubles {n, origin[3], sp, sq, spp, sqq,
 * spq, 0} to `dev_out` (device pointer, e.g. a row of a torch tensor that is
 * all-reduced over RCCL afterwards) without any host synchronisation. */
int  mvr_pair_moments2_dev(mvr_ctx *ctx, int src_slot, int tgt_slot, double max_dist,
                           int reciprocal, int fma_dist, size_t q_begin, size_t q_count,
                           const double origin[3], double *dev_out);
/* The whole edge list of one global iteration in one call (the `for` loops over
 * scan pairs of registrator.cpp:482-502 and :640-651): pair k = (src[k], dst[k])
 * with query range q_begin[k], q_count[k] (null arrays: all queries).  The pairs
 * are independent: with the culled search every stage (forward searches, flagging
 * of matched targets, reverse searches, filter + raw moments, final sums) is ONE
 * launch for all pairs (blockIdx.y = pair), six launches in all, so the pairs fill
 * the chip together; with the brute-force search (or pair_fused = 0) each pair runs
 * on one of `pair_streams` worker HIP streams forked from and joined back into the
 * context's stream (mvr_ctx_tune).  Results are identical to
 * n_pairs calls of mvr_pair_moments2.  out (host, [n_pairs]) and/or dev_out
 * (device, [n_pairs][32] doubles, no host synchronisation) receive the sums. */
int  mvr_pair_moments2_batch(mvr_ctx *ctx, int n_pairs, const int *src_slots, const int *tgt_slots,
                             double max_dist, int reciprocal, int fma_dist, const size_t *q_begin,
                             const size_t *q_count, const double origin[3],
                             mvr_pair_moments2_t *out, double *dev_out);

/* The accepted correspondences of pair k of the LAST fused mvr_pair_moments2_batch / mvr_ring_step on this context (the
 * culled / grid search with pair_fused, the default), as determineReciprocalCorrespondences lists them for that pair
 * (registrator.cpp:496-502, :644-649): ascending query index, squared distances; *m = number found (may exceed cap).
 * Read back from the keys the batch left on the device: valid until the next batch or any change of the pair's clouds
 * (MVR_E_ARG then).  What computeError shows and what the tests compare with the oracle's lists pair by pair. */
int  mvr_pair_batch_correspondences(mvr_ctx *ctx, int k, int32_t *query, int32_t *match, float *dist2, size_t cap, size_t *m);

/* ---- target sharding over ranks (sequential mode, registrator.cpp:563-577, is loop-carried and does not
 * shard by pair: the growing TARGET is split by points, every rank holds the full source).  A target slot
 * can be a shard: mvr_cloud_set_global_base / mvr_cloud_append_range record which GLOBAL point numbers its
 * local points carry.  One ICP iteration over G ranks is then
 *   mvr_nn_forward_keys        -> dev_keys[Ns] signed 64-bit (d2 bits << 32 | GLOBAL target index; INT64_MAX = none)
 *   all-reduce MIN over ranks    (RCCL ncclInt64/ncclMin: d2 >= 0, so signed order = (d2, index) order and
 *                                 ties go to the lowest global index -- the single-GPU rule)
 *   mvr_pair_moments2_from_keys -> this rank's share of the sums: reciprocal check, acceptance and raw
 *                                 second moments of the matches whose target point it OWNS (32 doubles,
 *                                 [31] = sum of d2), device output
 *   all-reduce SUM of the 32 doubles; then the usual host solve (mvr_moments_from_moments2 +
 *   mvr_umeyama_from_moments).  multi-view-registration_amd/seq.py is that loop. */
int  mvr_cloud_set_global_base(mvr_ctx *ctx, int slot, size_t global_begin);
int  mvr_cloud_append_range(mvr_ctx *ctx, int dst_slot, int src_slot, size_t src_begin, size_t count,
                            size_t global_begin);
int  mvr_nn_forward_keys(mvr_ctx *ctx, int src_slot, int tgt_slot, double max_dist, int fma_dist,
                         long long *dev_keys);
int  mvr_pair_moments2_from_keys(mvr_ctx *ctx, int src_slot, int tgt_slot, const long long *dev_keys,
                                 double max_dist, int reciprocal, int fma_dist, const double origin[3],
                                 double *dev_out);

/* The native host of that loop (csrc/mvr_align.hip, collectives in csrc/mvr_world.cpp).  mvr_seq_align_sharded: ONE
 * IterativeClosestPoint::align (registrator.cpp:569) of the full source in src_slot against the sharded target in tgt_slot
 * (this rank's shard), collectives on the context's communicator (mvr_ctx_comm_init / mvr_world_create; none = a world of
 * one): per iteration ncclAllReduce(ncclInt64, ncclMin) of the Ns keys and ncclAllReduce(ncclDouble, ncclSum) of the sums, on
 * the context's stream, then the host solve and the convergence criteria.  out_slot receives final * input (may equal
 * src_slot; < 0: none).  Every rank calls it with the same arguments and gets the same T_out / stats.
 * mvr_seq_run_sharded: Registrator::registrationICP (registrator.cpp:526-588) on top of it -- views 1, V-1, 2, ... aligned
 * one after the other against everything merged so far, pose_v <- T_icp * pose_v (:574), and `*target += aligned source`
 * (:576) as "every rank appends its slice [n g / G, n (g + 1) / G) of the aligned scan to its shard".  poses: n_views x 16
 * column-major, in / out; the per-align outputs (capacity repeat * (n_views - 1), any may be NULL) log the view, the
 * transformation and the statistics of every align.  PCL's "not enough correspondences" does not stop the driver
 * (registrator.cpp:569-574 never checks hasConverged()).
 * Failures: a rank whose local work fails still joins the iteration's collectives (neutral keys, zero sums, a raised failure
 * count), so every rank leaves the iteration together -- the failing one with its own status, the others with MVR_E_RCCL;
 * a rank whose peers never arrive gives up after "wait_timeout_ms" (mvr_ctx_tune), aborts the communicator
 * (ncclCommAbort) and returns MVR_E_RCCL.  The same holds for mvr_ring_run_sharded.  Never a hang. */
int  mvr_seq_align_sharded(mvr_ctx *ctx, int src_slot, int tgt_slot, int out_slot, const mvr_icp_params *params,
                           const double origin[3], float T_out[16], mvr_icp_stats *stats);
int  mvr_seq_run_sharded(mvr_ctx *ctx, int n_views, const int *raw_slots, int target_slot, int source_slot, int out_slot,
                         const mvr_icp_params *params, const double origin[3], int repeat, double *poses, int *align_view,
                         float *align_T, mvr_icp_stats *align_stats, int *n_aligns);
/* The same driver on ONE GPU around mvr_icp_align (Registrator::registrationICP, registrator.cpp:526-588, as one native call):
 * `repeat` sweeps; each poses view 0 into target_slot (reserved once for all the scans) and aligns views 1, V-1, 2, ... against
 * everything merged so far, pose_v <- T_icp * pose_v, target += aligned source.  poses: n_views x 16 column-major, in / out; the
 * per-align outputs as above (capacity repeat * (n_views - 1), any may be NULL).  MVR_E_NOCORR of an align does not stop it. */
int  mvr_seq_run(mvr_ctx *ctx, int n_views, const int *raw_slots, int target_slot, int source_slot, int out_slot,
                 const mvr_icp_params *params, int repeat, double *poses, int *align_view, float *align_T,
                 mvr_icp_stats *align_stats, int *n_aligns);

/* raw second moments of caller-supplied correspondences (lum.setCorrespondences,
 * registrator.cpp:650): query[k] indexes src_slot, match[k] indexes tgt_slot. */
int  mvr_pair_moments2_from_corr(mvr_ctx *ctx, int src_slot, int tgt_slot, const int32_t *query,
                                 const int32_t *match, size_t m, const double origin[3],
                                 mvr_pair_moments2_t *out);

/* host-side solves on the moments (3x3 SVD stays on the host) */
/* TransformationEstimationSVD / Eigen::umeyama (App. A.3). */
int  mvr_umeyama_from_moments(const mvr_pair_moments_t *mom, float T[16], double sv[3]);
int  mvr_moments_from_moments2(const mvr_pair_moments2_t *m2, mvr_pair_moments_t *out);

/* pcl::IterativeClosestPoint<PointXYZ,PointXYZ>::align(out)
 * (registrator.cpp:569, :920, :1012, :1024).  out_slot receives
 * final * input (may equal src_slot: the aliased align(*source_) of :920);
 * out_slot < 0 skips it.  T_out = getFinalTransformation().  Returns
 * MVR_E_NOCORR (and stats->state = NO_CORRESPONDENCES, converged = 0) when an
 * iteration finds < 3 correspondences; T_out then holds the transformation
 * accumulated so far, as PCL leaves it. */
int  mvr_icp_align(mvr_ctx *ctx, int src_slot, int tgt_slot, int out_slot,
                   const mvr_icp_params *params, float T_out[16], mvr_icp_stats *stats);

/* ---- correspondence rejectors (EXTENSION: pcl::registration::CorrespondenceRejector*, ICP::addCorrespondenceRejector) ------
 * What stands between the correspondence search of an ICP iteration and its estimator.  Views 30 degrees apart overlap only
 * partly: a fixed distance cap wide enough for the first iterations lets every rim point outside the overlap pull on the solve.
 * PCL was not at hand; the model is pcl/registration/correspondence_rejection_distance.h, _median_distance.h, _trimmed.h,
 * _surface_normal.h, _one_to_one.h (and their impl/ *.hpp) and pcl/registration/impl/icp.hpp, as published; deviations are marked.
 * Opt-in: mvr_icp_align, mvr_correspondences and every other entry keep their behaviour and their bits.
 *  R1. The table: a correspondence is (query i, match j, d2), d2 the f32 squared distance the search found; the chain never
 *      recomputes it (the rejectors carry no data container, which is what IterativeClosestPoint gives them).  Stages run in
 *      chain order, each sees only what the stage before kept.  LIVE = kept so far; m = the number live at a stage's entry.
 *  R2. DISTANCE: keep iff (double)d2 < value * value, strictly; the product is taken once on the host.
 *  R3. MEDIAN: med = the element at 0-based position m / 2 (integer division) of the live d2 in ascending order -- the upper
 *      median, what nth_element gives.  Keep iff (double)d2 <= (double)med * value.  With m == 0 nothing happens.
 *  R4. TRIMMED: nv = max((uint32_t)floor(value * (double)m), min_correspondences) (a product of 4294967295 or more counts as
 *      "all").  nv >= m keeps all.  Otherwise exactly the nv smallest by the key (d2 bits, query index) ascending are kept
 *      (nv == 0: none).  DEVIATION: PCL's nth_element leaves the choice among equal distances open; here the lower query
 *      index wins.
 *  R5. SURFACE_NORMAL: dot = (n.x * t.x + n.y * t.y) + n.z * t.z in f32, each operation rounded; n = the current source normal
 *      of i, t = the target normal of j.  Keep iff (double)dot > value; a NaN fails.  Both clouds must carry normals
 *      (mvr_cloud_upload_normals / mvr_cloud_estimate_normals), else MVR_E_ARG before any GPU work.
 *  R6. ONE_TO_ONE: among the live correspondences with the same match j the one with the smallest (d2 bits, query index) stays.
 *  R7. Output: the survivors in ascending query index (deterministic, where PCL's trimmed order is not).  *m may exceed cap:
 *      the lists are then truncated, as mvr_correspondences does.  stages[s] (optional, n_chain records) = the number live
 *      before and after stage s and the f32 d2 it cut at: MEDIAN the median, TRIMMED the largest d2 kept, both 0 when the
 *      stage had nothing to select from (m == 0, or nv == 0); 0 for the other kinds.  Bit-identical from run to run and for
 *      every launch shape: integer atomics only.
 *  R8. mvr_reject_correspondences runs the chain on the caller's list (query, match, dist2: host arrays of `count` entries):
 *      query indices below the source size and distinct, match indices below the target size, dist2 not NaN and >= 0 (+inf is
 *      allowed and sorts last); any violation is MVR_E_ARG with nothing written.  The slots are needed only for their sizes
 *      and, under R5, their normals.
 *  R9. mvr_icp_align_rejected is PCL's computeTransformation with rejectors.  Each iteration: the search of mvr_icp_align
 *      (max_corr_dist, use_reciprocal); the chain; fewer than 3 survivors: MVR_E_NOCORR with state NO_CORRESPONDENCES; the
 *      estimator (SVD, or point_to_plane) on the survivors; mse = the f64 sum of the survivors' f32 d2 / their number; the
 *      convergence criteria as in mvr_icp_align.  The current source of the next iteration is exactly what
 *      mvr_cloud_transform_f32 with the iteration's incremental transformation makes of the current one, points and (if
 *      present) normals, by the same kernels: PCL's incremental transformCloud.  T_out = the product of the incremental
 *      transformations by mvr_mat4f_mul.  trace[k] (optional, k < trace_cap) records iteration k.  With n_chain == 0 the
 *      result equals mvr_icp_align's in iterations / state / n_corr and in T within rounding (the sums run in another order,
 *      so the bits need not match).  Between the search and the sums nothing comes to the host: the chain rewrites the
 *      device's match table in place, and the counts and thresholds of its stages ride along with the iteration's sums.
 *      This holds for chains WITHOUT a SAMPLE_CONSENSUS stage: that stage (rules C1-C12 below) replays PCL's RANSAC loop on the
 *      host and costs round trips per chunk of attempts; its stage record still rides with the others.
 *  R10. MVR_E_ARG, before any GPU work and with nothing written, for a NULL ctx, a NULL chain with n_chain > 0, n_chain outside
 *      0..MVR_MAX_REJECTORS, an unknown kind, a non-finite value, a negative value of DISTANCE / MEDIAN / TRIMMED, a bad slot,
 *      a cloud above 0x7FFFFFF0 points or one whose points are stale because a pipelined run is in flight.  Empty clouds:
 *      MVR_OK with *m = 0.
 * Out of scope: CorrespondenceRejectorVarTrimmed, ...Features, ...OrganizedBoundary; SampleConsensus's isSampleGood; rejectors in
 * the ring / LUM passes, in mvr_seq_run, mvr_seq_align_sharded and the Registrator drivers. */
#define MVR_MAX_REJECTORS 8
enum { MVR_REJ_DISTANCE = 0, MVR_REJ_MEDIAN = 1, MVR_REJ_TRIMMED = 2, MVR_REJ_SURFACE_NORMAL = 3, MVR_REJ_ONE_TO_ONE = 4,
       MVR_REJ_SAMPLE_CONSENSUS = 5 };
typedef struct {
  int      kind;                 /* MVR_REJ_* */
  double   value;                /* DISTANCE: max distance (not squared); MEDIAN: factor; TRIMMED: overlap ratio;
                                    SURFACE_NORMAL: threshold (a cosine); ONE_TO_ONE: unused; SAMPLE_CONSENSUS: the inlier
                                    threshold (setInlierThreshold, not squared; PCL's default is 0.05) */
  uint32_t min_correspondences;  /* TRIMMED only */
  uint32_t max_iterations;       /* SAMPLE_CONSENSUS only: setMaximumIterations; 0 = PCL's 1000 */
  int      refine;               /* SAMPLE_CONSENSUS only: setRefineModel */
  uint64_t seed;                 /* SAMPLE_CONSENSUS only; ours: PCL draws with rand() */
} mvr_rejector;
typedef struct { uint32_t in, out; float threshold; } mvr_rejector_stage;
typedef struct {
  uint32_t n_found;                                /* correspondences the search found, before the chain */
  mvr_rejector_stage stages[MVR_MAX_REJECTORS];
  uint32_t n_corr;                                 /* survivors: what the estimator saw */
  double   mse;
  float    tr[16];                                 /* the iteration's incremental transformation (identity if none was solved) */
} mvr_icp_iter_trace;
int  mvr_correspondences_rejected(mvr_ctx *ctx, int src_slot, int tgt_slot, double max_dist, int reciprocal, int fma_dist,
                                  const mvr_rejector *chain, int n_chain, int32_t *query, int32_t *match, float *dist2,
                                  size_t cap, size_t *m, mvr_rejector_stage *stages /* n_chain, optional */);
int  mvr_reject_correspondences(mvr_ctx *ctx, int src_slot, int tgt_slot, const int32_t *query, const int32_t *match,
                                const float *dist2, size_t count, const mvr_rejector *chain, int n_chain, int32_t *q_out,
                                int32_t *m_out, float *d_out, size_t cap, size_t *m, mvr_rejector_stage *stages);
int  mvr_icp_align_rejected(mvr_ctx *ctx, int src_slot, int tgt_slot, int out_slot, const mvr_icp_params *params,
                            const mvr_rejector *chain, int n_chain, float T_out[16], mvr_icp_stats *stats,
                            mvr_icp_iter_trace *trace /* optional */, int trace_cap);

/* ---- the sample-consensus rejector (EXTENSION: pcl::registration::CorrespondenceRejectorSampleConsensus) -------------------
 * The one rejector that knows about the transformation: it keeps the correspondences that agree with ONE rigid motion, found by
 * RANSAC over the correspondences themselves.  It is kind MVR_REJ_SAMPLE_CONSENSUS of a chain (any position, more than once) in
 * mvr_correspondences_rejected, mvr_reject_correspondences, mvr_icp_align_rejected and mvr_icp_align_gicp, and it has an entry of
 * its own that returns the full evidence.  The slots supply the points: in the two align entries the source is the CURRENT source
 * of the iteration (what PCL's ICP hands over with setSourcePoints), in the list entries the source slot as it stands.  PCL was
 * not at hand; the model is pcl/registration/impl/correspondence_rejection_sample_consensus.hpp,
 * pcl/sample_consensus/impl/sac_model_registration.hpp and ransac.hpp, as published; deviations are marked.  Every f32 operation
 * is rounded on its own and never contracted.
 *  C1. The list L = the live correspondences (i, j, d2) in ascending query index, m of them.  A pair is VALID when p_i and q_j
 *      both have three finite coordinates; nv = the number valid.  An invalid pair is never sampled and never an inlier.
 *      nv < 3: found = 0 and no attempt is made.
 *  C2. Draws: rule P2 unchanged over the valid pairs in ascending query index; sample r is the r-th valid pair.  The three are
 *      distinct by construction.  DEVIATION: PCL's rand(), its isSampleGood spread test and its retry loop are not reproduced.
 *  C3. Hypothesis: rule A5's estimator on the three pairs in sample order -- f64 means and covariance, the host SVD of
 *      mvr_umeyama_from_moments (Eigen::umeyama without scaling), cast to f32.  The attempt is SKIPPED (status 0; its traced T
 *      and count are 0) when any entry of T is non-finite.  The attempts of a chunk are drawn and their sample coordinates
 *      gathered by one launch, solved on the host and uploaded as one block.
 *  C4. Transformed point: mvr_cloud_transform_f32's arithmetic on p_i: x' = ((T00 x + T01 y) + T02 z) + T03, and so for y', z'.
 *  C5. d2 = (dx dx + dy dy) + dz dz in f32 with d = p' - q_j, q_j the pair's OWN match (no search); with fma_dist
 *      d2 = fmaf(dz, dz, fmaf(dy, dy, dx dx)) as everywhere.  fma_dist is the entry's argument or params; in
 *      mvr_reject_correspondences and mvr_reject_sample_consensus, which have none, the non-fma form is the rule.  The pair is
 *      an inlier iff (double)d2 < value * value, strictly; the product is taken once on the host (the kernels compare with the
 *      smallest f32 that is >= it, which is the same test).
 *  C6. The count of an attempt is the exact integer number of inliers: independent of order and of launch shape.
 *  C7. The loop is P7 verbatim with this nv: strictly greater, w = best_count / (double)nv, pno = 1 - w^3 clamped, probability
 *      0.99 (fixed, as in the PCL class), PCL's off-by-one of max_iterations + 1 counted attempts, skipped < 10 * max_iterations.
 *      It is replayed on the host over a chunk's counts; the attempts beyond the stop are discarded.  Tune key "rej_sac_chunk":
 *      1..256 attempts per chunk; 0 (default) = the library's choice.  Result and trace are bit-identical for every chunk size.
 *  C8. found = (best_count >= 3).  Not found: PCL returns the original list; here the stage keeps every live entry, invalid ones
 *      included: out = in, T = identity, best_attempt = -1.
 *  C9. Found: the survivors are exactly the C5 inliers of the best attempt's T; every other entry gets match = -1.
 *  C10. refine (setRefineModel).  DEVIATION from PCL's sigma / variance loop.  T_0 = the RANSAC T, I_0 = its inliers.  Round
 *      r >= 1: T_r = the ICP SVD estimator over I_{r-1} -- the fixed-order f64 raw moments the align entries sum over the match
 *      table (taken about the target point of the best attempt's first sample), mvr_moments_from_moments2, the host SVD, cast
 *      to f32 --; I_r = C5 with T_r over all valid live pairs.  |I_r| < 3 or a non-finite T_r: stop with (T_{r-1}, I_{r-1}).
 *      I_r = I_{r-1} as sets, or r = max_iterations (PCL's cap): stop with (T_r, I_r).  refine_rounds = the r reached.
 *      ransac_T and ransac_inliers always record T_0 and |I_0|.
 *  C11. Outputs follow R7: ascending query index, truncated at cap.  result: live = m, valid = nv, inliers = the survivors
 *      (= m when not found).  trace[t] (optional) for every attempt made, t < trace_cap: status (0 skipped, 1 counted), the
 *      sampled pairs' query and match indices, T, the count and k after the attempt.  The stage record is in, out, threshold 0.
 *  C12. MVR_E_ARG, before any GPU work and with nothing written: everything of R8 and R10; a value that is not finite and > 0;
 *      max_iterations above 1 << 24; a NULL rejector / result / m, or a rejector of another kind, in the dedicated entry.  Empty
 *      clouds or lists: MVR_OK with found = 0 (T = identity).  Bit-identical from run to run: integer atomics only, every f64
 *      sum in a fixed order.
 * mvr_ctx_last_sample_consensus: the result of the last SAMPLE_CONSENSUS stage that ran on this context, inside any of the
 * entries above (what getBestTransformation() reads after an align); MVR_E_ARG when none has run. */
typedef struct { int found; uint32_t live, valid, inliers, ransac_inliers;
                 int iterations, attempts, skipped, best_attempt, refine_rounds;
                 double k; float T[16], ransac_T[16]; } mvr_rej_sac_result;      /* T: column-major 4 x 4 */
typedef struct { int status; uint32_t query[3], match[3]; float T[16]; uint32_t inliers; double k; } mvr_rej_sac_trace;
int  mvr_reject_sample_consensus(mvr_ctx *ctx, int src_slot, int tgt_slot, const int32_t *query, const int32_t *match,
                                 const float *dist2, size_t count, const mvr_rejector *r, mvr_rej_sac_result *result,
                                 int32_t *q_out, int32_t *m_out, float *d_out, size_t cap, size_t *m,
                                 mvr_rej_sac_trace *trace /* optional */, size_t trace_cap);
int  mvr_ctx_last_sample_consensus(mvr_ctx *ctx, mvr_rej_sac_result *result);

/* ---- Generalized ICP (EXTENSION: pcl::GeneralizedIterativeClosestPoint) ----------------------------------------------------
 * Plane-to-plane ICP: every correspondence is weighed by the surface each of its two points lies on, so two scans that sample
 * the same surface at different points -- every pair of turntable views -- are not pulled point onto point.  PCL was not at
 * hand; the model is pcl/registration/gicp.h and impl/gicp.hpp as published; deviations are marked.  Opt-in: no other entry
 * changes.
 *  G1. Inputs: both slots carry normals (mvr_cloud_upload_normals / mvr_cloud_estimate_normals), else MVR_E_ARG before any GPU
 *      work, as under R5.  A normal is used as a direction only: neither its sign nor its length matters.  PCL's regularised
 *      covariance of a k-neighbourhood (eigenvalues 1, 1, eps along its principal directions) is exactly I - (1 - eps) n n^T
 *      with n the eigenvector of the smallest eigenvalue, which is what mvr_cloud_estimate_normals in k mode leaves.
 *  G2. An outer iteration: the search of mvr_icp_align_rejected (max_corr_dist, use_reciprocal, fma_dist); the rejector chain
 *      (R1-R7); fewer than 3 live correspondences: MVR_E_NOCORR with state NO_CORRESPONDENCES; the inner optimisation (G5-G7)
 *      over the live correspondences (i, j) with the current source points p_i and normals s_i and the target's q_j and n_j.
 *  G3. Side matrices, all arithmetic in f64.  n^ = n / |n| when the three components are finite and |n|^2 > 0.
 *      A_i = I - (1 - eps) s^ s^T, B_j = I - (1 - eps) n^ n^T, eps = gicp_epsilon in (0, 1] (PCL: 0.001).  A side whose normal
 *      fails the test takes I: the library's rule (PCL has no such case, its covariances come from neighbourhoods).
 *  G4. W_i = (A_i + B_j)^-1, fixed for the whole inner optimisation: the current normals already carry the rotation
 *      accumulated so far, which is PCL's R C_s R^T + C_t.  A + B has eigenvalues in [2 eps, 2]; the inverse is the closed-form
 *      symmetric one (cofactors over the determinant) in f64.  Its accuracy is about 5e-16 / eps relative to |W|; nothing is
 *      promised below eps = 1e-9.
 *  G5. The objective at X = (R, t): F = (1 / m) sum r^T W r, y = R p + t, r = y - q.  Linearised by y' = Exp(w) y + v,
 *      delta = (w, v), rotation first as in the point-to-plane row: J = [-[y]x | I].  The 29 sums: 0..20 the upper triangle of
 *      H = sum J^T W J, row-major; 21..26 g = sum J^T W r; 27 the count m; 28 f = sum r^T W r.  f64, in a fixed order,
 *      bit-identical from run to run: block partials and a one-block final sum, as the point-to-plane sums.
 *  G6. A step: (H + lambda diag(H)) delta = -g by a 6x6 Cholesky in f64; a pivot that is <= 0 or not finite ends the
 *      optimisation with MVR_E_SINGULAR.  The candidate is R_c = E R, t_c = E t + v, E the Rodrigues matrix of w
 *      (|w| < 1e-8: I + K + K^2 / 2, K = [w]x).  (The damping makes the system positive definite whenever diag(H) > 0: a
 *      rank-deficient H is caught here only when a diagonal entry is 0, e.g. every point at the origin; otherwise by G7's
 *      lambda > 1e9.)
 *  G7. The inner loop is Levenberg-Marquardt.  DEVIATION: PCL runs BFGS on (x, y, z, roll, pitch, yaw); the objective is the
 *      same and so is its minimum.  Start at X = I with lambda = 1e-3 and evaluate G5 there.  If f there is not finite -- a
 *      listed point or an entry of a W is NaN or infinite -- the optimisation ends with MVR_E_SINGULAR, evaluations = 1 and
 *      X = I (the searches never match a non-finite point; a caller's list may name one).  While evaluations <
 *      max_inner_iterations (PCL: 20): step by G6, evaluate at the candidate, decide.  ACCEPT when f_c < f (strictly; a NaN
 *      fails): X and the sums become the candidate's, lambda = max(lambda / 10, 1e-9), and the loop ends when |w|_2 <
 *      inner_rot_tol (default 1e-6 rad) and |v|_2 < inner_trans_tol (default 1e-5).  REJECT otherwise: lambda = 10 lambda,
 *      and the loop ends when lambda > 1e9.  The loop runs on the device: the host queues inner_chunk evaluation + step pairs
 *      behind each other and reads the state once per chunk (0: all max_inner_iterations at once; default 4); a pair queued behind the
 *      end does nothing, so the result is bit-identical for every inner_chunk.
 *  G8. The outer step: tr = X rounded to f32; fin = tr * fin by mvr_mat4f_mul; the current source moves exactly as in R9,
 *      points and normals.  delta = the largest of |fin_new - fin_old| / rotation_epsilon over the 3x3 block and
 *      |fin_new - fin_old| / transformation_epsilon over the translation column, taken in f64 from the f32 entries (PCL:
 *      rotation_epsilon 2e-3, transformation_epsilon 5e-4, max_iterations 200, max_corr_dist 5).  ++iterations; delta < 1:
 *      MVR_CONV_TRANSFORM; else iterations >= max_iterations: MVR_CONV_ITERATIONS; both with converged = 1, as PCL.  mse = the
 *      mean of the survivors' f32 d2, as in R9.
 *  G9. out_slot, T_out and the stats as in mvr_icp_align_rejected.  trace[k] (optional, k < trace_cap) records iteration k.
 *  G10. All of R10; also MVR_E_ARG before any GPU work, with nothing written, for gicp_epsilon outside (0, 1], an epsilon or
 *      a tolerance that is not positive and finite (transformation_epsilon, rotation_epsilon, inner_rot_tol, inner_trans_tol),
 *      max_inner_iterations < 1.  An inner_chunk below 1 or above max_inner_iterations counts as 0.  Empty clouds follow R9
 *      and R10.
 * mvr_gicp_sums / mvr_gicp_solve are G5 and G5-G7 on the caller's correspondence list (query / match: host arrays of `count`
 * entries, validated as in R8; the slots supply points and normals).  X, X_out: 4x4 column-major f64.  mvr_gicp_solve
 * returns MVR_E_NOCORR for fewer than 3 entries and MVR_E_SINGULAR as G6 and G7; X_out and info hold the state reached.
 * mvr_gicp_sums has no such rule: on a list that names a non-finite point it returns MVR_OK, the exact count in out[27] and
 * sums that are not finite.
 * Out of scope: PCL's BFGS; setSourceCovariances / setTargetCovariances; GICP in the ring / LUM passes, in mvr_seq_run, the
 * sharded entries and the Registrator drivers. */
typedef struct {
  double max_corr_dist;            /* setMaxCorrespondenceDistance (PCL's GICP: 5)                                      */
  int    use_reciprocal;           /* setUseReciprocalCorrespondences                                                   */
  int    fma_dist;
  int    max_iterations;           /* setMaximumIterations (PCL's GICP: 200)                                            */
  int    max_inner_iterations;     /* setMaximumOptimizerIterations: evaluations of the objective per outer iteration   */
  double transformation_epsilon;   /* setTransformationEpsilon (PCL's GICP: 5e-4)                                       */
  double rotation_epsilon;         /* setRotationEpsilon (2e-3)                                                         */
  double gicp_epsilon;             /* the small eigenvalue of the side covariances (0.001)                              */
  double inner_rot_tol;            /* G7: an accepted step below both tolerances ends the inner loop                    */
  double inner_trans_tol;
  int    inner_chunk;              /* evaluation + step pairs queued per host round trip; 0 = max_inner_iterations;
                                      default 4, the fastest of 1 / 4 / 0 on the 200k view pair (profiles/gicp_bench.json)     */
} mvr_gicp_params;
void mvr_gicp_default_params(mvr_gicp_params *p);
typedef struct {
  uint32_t n_found;                                /* correspondences the search found, before the chain */
  mvr_rejector_stage stages[MVR_MAX_REJECTORS];
  uint32_t n_corr;                                 /* survivors: what the optimiser saw */
  double   mse;
  double   f0, f1;                                 /* the objective per correspondence at identity and at X */
  uint32_t inner_evals, inner_accepted;
  double   lambda;
  float    tr[16];                                 /* X rounded to f32 (identity if none was solved) */
} mvr_gicp_iter_trace;
typedef struct {
  uint32_t evaluations, accepted;
  double   lambda, f0, f1;
} mvr_gicp_info;
int  mvr_icp_align_gicp(mvr_ctx *ctx, int src_slot, int tgt_slot, int out_slot, const mvr_gicp_params *params,
                        const mvr_rejector *chain, int n_chain, float T_out[16], mvr_icp_stats *stats,
                        mvr_gicp_iter_trace *trace /* optional */, int trace_cap);
int  mvr_gicp_sums(mvr_ctx *ctx, int src_slot, int tgt_slot, const int32_t *query, const int32_t *match, size_t count,
                   const double X[16], double gicp_epsilon, double out[29]);
int  mvr_gicp_solve(mvr_ctx *ctx, int src_slot, int tgt_slot, const int32_t *query, const int32_t *match, size_t count,
                    const mvr_gicp_params *params, double X_out[16], mvr_gicp_info *info);

/* ---- Normal Distributions Transform (EXTENSION: pcl::NormalDistributionsTransform) -----------------------------------------
 * Registration without a correspondence search: the source is scored against one Gaussian per voxel of the target and the
 * pose takes Newton steps on that score.  The voxel size sets the basin, not a nearest-neighbour cap.  PCL was not at hand;
 * the model is pcl/registration/ndt.h, impl/ndt.hpp and pcl/filters/voxel_grid_covariance.h as published; deviations are
 * marked.  Opt-in: no other entry changes.  resolution, step_size and transformation_epsilon are in the cloud's unit (PCL's
 * defaults are meant for metres).
 *  N1. Inputs: a source slot and a target slot, points only.  A non-finite target point belongs to no voxel (voxel rule 1); a
 *      non-finite source point contributes nothing.  All arithmetic after the f32 voxel index is f64.
 *  N2. Constants, as PCL's init(): c1 = 10 (1 - outlier_ratio), c2 = outlier_ratio / resolution^3, d3 = -log c2,
 *      d1 = -log(c1 + c2) - d3, d2 = -2 log((-log(c1 exp(-1/2) + c2) - d3) / d1).
 *  N3. Cells.  The voxel index is rules 2-4 of mvr_cloud_voxel_grid with leaf = (float)resolution on all three axes; where rule
 *      3 would pass the cloud through (lattice too large) the call returns MVR_E_ARG.  A voxel with n >= min_points_per_voxel
 *      (default 6, as PCL; values below 3 count as 3) gets its mean m = (sum p) / n, kept in f64, and
 *      C = ((n - 1) / n) (1 / n) sum (p - m)(p - m)^T -- centred, two passes, fixed order; PCL's uncentred expression has the
 *      same value, and the odd (n - 1) / n is PCL's.  C is eigen-decomposed by the cyclic Jacobi of the normals; lmax = the
 *      largest eigenvalue.  The voxel is dropped when lmax is not finite or <= 0.  l'_k = max(l_k, min_covar_eigvalue_mult
 *      lmax) (default 0.01), C^-1 = V diag(1 / l') V^T.  DEVIATION: PCL rebuilds C and inverts it numerically.  Kept cells are
 *      stored in ascending voxel index: key, n, m[3], C^-1 (xx xy xz yy yz zz).  A wave sums a voxel (lane l takes sorted
 *      positions l, l + 64, ...; then a fixed-order wave sum), so a long voxel is not serialised on one thread.
 *  N4. Pose p = (tx, ty, tz, rx, ry, rz): y = R(r)(x - o) + o + t, R = Rx(rx) Ry(ry) Rz(rz) as PCL; x = G x_raw with G the
 *      optional 4x4 f64 guess (NULL: I), applied in f64 at every evaluation: the raw source is never re-rounded.  o = origin[3]
 *      is an EXTENSION (PCL rotates about the frame's origin, o = 0, the default): far from the origin the rotation and
 *      translation parameters are strongly coupled and the line search of N8 wanders.  DEVIATION: PCL parametrises the guess
 *      itself by Euler angles; here p is the increment on top of G and the result is X(p) G.  No small-angle shortcut (PCL
 *      zeroes sines below 1e-5).
 *  N5. Neighbourhood.  The home voxel of y is h[a] = floor((float)y[a] inv) - min_b[a] by the f32 rule of the voxel index.  The
 *      candidates are the 27 voxels h + {-1, 0, 1}^3 that lie inside the lattice and hold a kept cell, visited in ascending
 *      voxel index.  A candidate counts when |y - m|^2 <= resolution^2 in f64 (PCL: radiusSearch over the centroids, in f32).
 *      DEVIATION: a centroid within the radius whose voxel is not one of the 27 is not seen (it cannot happen for a centroid
 *      inside its own voxel and a y inside its home voxel, up to f32 rounding of the index).
 *  N6. The 29 sums, over every counted pair (point, cell): d = y - m, v = C^-1 d, q = d.v, e = exp(-d2 q / 2), w = d2 e.  A
 *      pair with !(0 <= w <= 1) -- PCL's guard; a NaN too -- is skipped whole and is not counted.  J = [I | D1 x~, D2 x~, D3 x~],
 *      x~ = x - o, D_k = dR/dr_k; K_ij = (d2R / dr_i dr_j) x~ for angular i, j, else 0; a_i = v.J_i.  Per pair:
 *      s += -d1 e; g_i += d1 w a_i; H_ij += d1 w (J_i^T C^-1 J_j - d2 a_i a_j + v.K_ij).  The host forms R, the D_k and the six
 *      second-derivative matrices in f64 as products of the axis rotations and their angle derivatives (the angle shifted by
 *      pi/2 per derivative order, the constant entries zeroed).  Layout, as G5: 0..20 the upper triangle of H, row-major;
 *      21..26 g; 27 the number of counted pairs; 28 s.  Fixed order, bit-identical from run to run.  s is to be MAXIMISED.
 *  N7. Direction: delta = -H^+ g from a cyclic Jacobi eigen-decomposition of the symmetric 6x6 H on the host, in f64;
 *      eigenvalues with |l| <= 6 * 2^-52 * max|l| are dropped (Eigen's default JacobiSVD threshold, which PCL's solve uses).
 *      A non-finite entry of H or g makes delta not a number.  |delta| 0 or not finite: stop MVR_NDT_FLAT.  u = delta /
 *      |delta|, phi'0 = -g.u; phi'0 > 0: u = -u, phi'0 = -phi'0 (PCL's reversal); phi'0 == 0: stop MVR_NDT_FLAT.
 *  N8. Step length.  DEVIATION: PCL runs More-Thuente with interpolation and a curvature condition; here it is backtracking
 *      with PCL's mu = 1e-4 and PCL's bounds.  a = min(|delta|, step_size).  Up to max_line_evals trials (default 10, PCL's
 *      max_step_iterations), each: evaluate N6 at p + a u; accept at the first trial with -s(a) <= -s(0) + mu a phi'0;
 *      otherwise remember the trial with the largest s among those with s(a) > s(0); then halve a and leave the loop when
 *      a < transformation_epsilon / 2.  No trial accepted: the remembered one is taken with its own a (the trace's `fallback`);
 *      none remembered: stop MVR_NDT_NO_DECREASE with the pose as it was.  (The score is only piecewise smooth, cells enter
 *      and leave the radius, and plain Armijo stalls short of the optimum.)
 *  N9. Stops.  After a taken step p += a u and ++iterations; the sums of the taken trial become the current ones (no
 *      re-evaluation).  a < transformation_epsilon: MVR_NDT_STEP, converged.  iterations >= max_iterations:
 *      MVR_NDT_ITERATIONS, converged, as PCL.  A count of 0 at the starting pose (an empty source or cell set too):
 *      MVR_E_NOCORR with stop MVR_NDT_NO_OVERLAP and T = G.  DEVIATION: PCL never stops on its first iteration.  PCL's
 *      defaults: resolution 1, step_size 0.1, outlier_ratio 0.55, transformation_epsilon 0.1, max_iterations 35.
 *      The loop of N7-N9 is mvr_ndt_newton, host code that takes the evaluation of N6 as a callback: mvr_ndt_align passes the
 *      GPU's, a test may pass a script.  The order of the stops is: STEP before ITERATIONS (a short last step says STEP).
 *  N10. Outputs: X_out = X(p) G, f64 4x4 column-major; T_out the same rounded to f32; out_slot (-1: none) = the source under
 *      T_out, exactly as the other aligns write theirs.  Stats: iterations, stop, converged, evaluations, n_cells, n_pairs
 *      (sum 27 at the end), score, ms.  trace[k], k < trace_cap: a, |delta|, trials, the reversed and fallback flags, score,
 *      count and p[6] after iteration k (an iteration that stopped without a step records the pose as it was).  A trace_cap
 *      shorter than the run changes nothing else: records from trace_cap on are not written.
 *  N11. MVR_E_ARG before any GPU work, with nothing written, for: a NULL ctx or params, a bad slot, an output slot equal to
 *      the source or the target slot; a resolution, step_size, transformation_epsilon or min_covar_eigvalue_mult that is not finite and
 *      > 0; an outlier_ratio outside (0, 1); d1 or d2 not finite, d1 >= 0 or d2 <= 0; max_iterations < 1 or max_line_evals < 1;
 *      a non-finite origin or G.  mvr_ndt_constants runs exactly these parameter checks on the host (no context) and returns
 *      d1, d2, d3.
 *  N12. The cells are built once per call and live in the context's scratch arena; nothing is cached on a slot.
 * Lookup: a dense uint32 table voxel -> cell when the lattice has at most "ndt_dense_max" entries (mvr_ctx_tune, default
 * 1 << 24; 0 forces the other route), else a binary search of the kept keys per (j, k) row; both give the same bits.
 * mvr_ndt_cells builds the cells of a target and downloads them (host arrays optional, `cap` entries each; *n = the number of
 * cells).  mvr_ndt_sums is N6 at the pose p.  mvr_ndt_direction is N7 on the host: MVR_OK with delta[6], or MVR_E_SINGULAR
 * where N7 says FLAT on |delta|.  mvr_ndt_newton runs N7-N9 from p = 0 on the sums `eval` returns (0: fine; anything else is
 * returned at once, with no output written): p_out, sums_out (optional: the sums at p_out), the stats' iterations, stop,
 * converged, evaluations, n_pairs and score (n_cells and ms are left alone) and the trace; it returns MVR_OK, MVR_E_NOCORR
 * (stop MVR_NDT_NO_OVERLAP) or MVR_E_ARG (N11's parameter checks, a NULL params, eval or p_out).  No context, no GPU.
 * Out of scope: More-Thuente interpolation, a device-side Newton loop, cached cells, NDT in the ring / sequential / sharded
 * drivers, multi-resolution schedules. */
enum { MVR_NDT_NOT = 0, MVR_NDT_STEP = 1, MVR_NDT_ITERATIONS = 2, MVR_NDT_FLAT = 3, MVR_NDT_NO_DECREASE = 4, MVR_NDT_NO_OVERLAP = 5 };
typedef struct {
  double resolution;               /* setResolution: the voxel edge (PCL: 1)                                             */
  double step_size;                /* setStepSize: the longest step of the line search (0.1)                             */
  double outlier_ratio;            /* setOulierRatio (0.55)                                                              */
  double transformation_epsilon;   /* setTransformationEpsilon (0.1)                                                     */
  double min_covar_eigvalue_mult;  /* VoxelGridCovariance::setMinimumPointNumberPerVoxel's companion (0.01)              */
  double origin[3];                /* N4: the point the rotation turns about (0, 0, 0)                                   */
  int    max_iterations;           /* setMaximumIterations (35)                                                          */
  int    max_line_evals;           /* N8: trials per line search (10)                                                    */
  int    min_points_per_voxel;     /* setMinPointPerVoxel (6; below 3 counts as 3)                                       */
} mvr_ndt_params;
void mvr_ndt_default_params(mvr_ndt_params *p);
typedef struct {
  int      iterations, stop /* MVR_NDT_* */, converged, evaluations;
  uint32_t n_cells;
  double   n_pairs, score, ms;
} mvr_ndt_stats;
typedef struct {
  double a, delta_norm;
  int    trials, reversed, fallback, stop;
  double score, count, p[6];
} mvr_ndt_iter_trace;
int  mvr_ndt_constants(const mvr_ndt_params *params, const double *guess /* optional, 16 */, double d123[3]);
int  mvr_ndt_direction(const double sums[29], double delta[6]);
typedef int (*mvr_ndt_eval_fn)(void *user, const double p[6], double sums[29]);
int  mvr_ndt_newton(const mvr_ndt_params *params, mvr_ndt_eval_fn eval, void *user, double p_out[6], double sums_out[29],
                    mvr_ndt_stats *stats, mvr_ndt_iter_trace *trace /* optional */, int trace_cap);
int  mvr_ndt_cells(mvr_ctx *ctx, int tgt_slot, const mvr_ndt_params *params, size_t cap, uint64_t *key, uint32_t *count,
                   double *mean /* 3 per cell */, double *icov /* 6 per cell */, size_t *n);
int  mvr_ndt_sums(mvr_ctx *ctx, int src_slot, int tgt_slot, const mvr_ndt_params *params, const double *guess /* optional, 16 */,
                  const double p[6], double out[29]);
int  mvr_ndt_align(mvr_ctx *ctx, int src_slot, int tgt_slot, int out_slot, const mvr_ndt_params *params,
                   const double *guess /* optional, 16 */, float T_out[16], double X_out[16], mvr_ndt_stats *stats,
                   mvr_ndt_iter_trace *trace /* optional */, int trace_cap);

/* Registration::getFitnessScore(max_range) (registrator.cpp:572,923,1015):
 * mean squared distance of T*input to its unbounded 1-NN in the target.
 * DBL_MAX when no point qualifies. */
int  mvr_fitness(mvr_ctx *ctx, int input_slot, int tgt_slot, const float T[16],
                 double max_range, int fma_dist, double *score);

/* ---- LUM (pcl::registration::LUM, registrator.cpp:627-663) ------------------- */
/* LUM::computeEdge for one edge from its raw moments and the two vertex poses
 * (x,y,z,roll,pitch,yaw): MM (6x6 row-major), MZ, ss, n_valid. */
int  mvr_lum_edge_from_moments(const mvr_pair_moments2_t *m2, const double pose_s[6],
                               const double pose_t[6], double MM[36], double MZ[6],
                               double *ss);
/* The same for FOUR edges in one pass (one per AVX2 lane; what mvr_lum_compute runs its edges through): m2[4],
 * pose_s / pose_t [4][6], MM [4][36], MZ [4][6], ss [4].  Bit-identical to four calls of the function above;
 * MVR_E_NOCORR (outputs untouched) when a lane needs one of its special paths (n < 3, an unsafe Cholesky pivot). */
int  mvr_lum_edge_from_moments_x4(const mvr_pair_moments2_t *m2, const double *pose_s, const double *pose_t,
                                  double *MM, double *MZ, double *ss);
/* LUM::compute on n vertices / ne edges given per-edge moments; poses n*6
 * in/out, vertex 0 fixed.  Returns iterations done in *iters. */
int  mvr_lum_compute(int n, int ne, const int *edge_src, const int *edge_tgt,
                     const mvr_pair_moments2_t *edge_m2, int max_iterations,
                     double convergence_threshold, double *poses, int *iters);
/* the host side of one global step of registrationLUM (registrator.cpp:650-662)
 * from the (all-reduced) ne x 32 edge table: per-pair Umeyama + residual,
 * LUM::compute, pose_v <- LUM_v * pose_v (poses: n_views x 16 column-major,
 * in/out; vertex 0 fixed).  pair_T (ne x 16) may be NULL. */
int  mvr_ring_host_step(int n_views, int ne, const int *edge_src, const int *edge_tgt, const double *rows,
                        const double origin[3], int lum_iterations, double *poses, double *lum_pose,
                        float *pair_T, double *pair_n, double *pair_mse, int *lum_iters);
/* One outer pass of Registrator::registrationLUM (registrator.cpp:625-664) in ONE call, for a single process:
 *   posed_slots[v] <- poses[v] applied to raw_slots[v]            (mvr_cloud_transform_batch)
 *   per edge e: reciprocal correspondences of posed[edge_src[e]] in posed[edge_tgt[e]] + raw moments
 *                                                                 (mvr_pair_moments2_batch)
 *   host: per-pair Umeyama + residual, LUM::compute, pose_v <- LUM_v * pose_v   (mvr_ring_host_step)
 * edge_src / edge_tgt are VIEW indices (0..n_views-1).  poses: n_views x 16 column-major, in/out.  Optional
 * outputs (may be NULL): rows (ne x 32, the edge table as mvr_pair_moments2_dev lays it out), pair_T (ne x 16),
 * timing_ms[3] = {enqueue, wait for the GPU + copy of the table, host solve}.  Synchronises the context's stream. */
int  mvr_ring_step(mvr_ctx *ctx, int n_views, const int *posed_slots, const int *raw_slots, int ne, const int *edge_src,
                   const int *edge_tgt, double max_dist, int reciprocal, int fma, const double origin[3], int lum_iterations,
                   double *poses, double *lum_pose, float *pair_T, double *pair_n, double *pair_mse, int *lum_iters,
                   double *rows, double *timing_ms);
/* n_steps outer passes (the loop of registrator.cpp:625-664), each exactly one mvr_ring_step; the outputs are those
 * of the LAST pass, timing_ms the SUM over the passes.  Stops at the first pass that fails and returns its status.
 * (pair_T is computed for the last pass only -- a 3 x 3 SVD per pair that no pass in between needs: it is left untouched when
 * the run stops early; pair_n, pair_mse, lum_pose and rows are those of the last pass that was solved.)
 * In steady state (no allocation, no index or grid to build: from the third or fourth pass of a registration on) the
 * passes are PIPELINED: the launch chain of pass k+1 is queued behind a gate while pass k runs and released by the host's
 * solve with one store (tune key "pipeline"); same results, bit for bit. */
int  mvr_ring_run(mvr_ctx *ctx, int n_steps, int n_views, const int *posed_slots, const int *raw_slots, int ne,
                  const int *edge_src, const int *edge_tgt, double max_dist, int reciprocal, int fma, const double origin[3],
                  int lum_iterations, double *poses, double *lum_pose, float *pair_T, double *pair_n, double *pair_mse,
                  int *lum_iters, double *rows, double *timing_ms);
/* LUM::incidenceCorrection(pose) (inside lum.compute(), registrator.cpp:654): the 6x6 (row-major) matrix H with
 * d(R p + t)/d pose = M(p') H for R = Rx Ry Rz and the M of LUM::computeEdge; exposed so that its sign pattern can be
 * pinned by a numeric Jacobian without a GPU. */
void mvr_lum_incidence(const double pose[6], double H[36]);
/* ---- multi-GPU: the outer passes of registrationLUM (registrator.cpp:625-664) sharded over the GPUs of one node ----
 * The shardable unit is the scan pair of the loop at registrator.cpp:640-651.  The V * Ns source queries of all pairs
 * are dealt to the ranks in contiguous equal ranges (mvr_ring_segments; a pair may be split between two ranks, its
 * sums are additive); every rank holds every scan, no point crosses the fabric.  Per pass each rank runs its share
 * of the fused searches + sums, then ONE ncclAllReduce(sum) of the [edges][32] f64 table over RCCL/xGMI on the
 * context's stream, then the (tiny) host solve -- redundantly on every rank from identical bits, so no broadcast.
 * RCCL is loaded at run time (dlopen: a copy the process already holds, e.g. PyTorch-ROCm's, else the system one,
 * else $MVR_RCCL_LIB); without it these entry points return MVR_E_RCCL and nothing else is affected.
 *
 * (a) one process per GPU (the usual launcher shape): rank 0 calls mvr_comm_unique_id, the 128 bytes travel to the
 *     other ranks by the launcher's own means, every rank calls mvr_ctx_comm_init on its context, then all ranks
 *     call mvr_ring_run_sharded with the same arguments.  A context without a communicator is a world of one
 *     (mvr_ring_run_sharded == mvr_ring_run). */
#define MVR_UNIQUE_ID_BYTES 128
int  mvr_comm_unique_id(char id[MVR_UNIQUE_ID_BYTES]);
int  mvr_ctx_comm_init(mvr_ctx *ctx, const char id[MVR_UNIQUE_ID_BYTES], int rank, int world);   /* ncclCommInitRank: collective */
int  mvr_ctx_comm_destroy(mvr_ctx *ctx);
/* rank / world of the context and the rank count RCCL itself reports for its communicator (0: none) */
int  mvr_ctx_comm_info(mvr_ctx *ctx, int *rank, int *world, int *rccl_ranks);
const char *mvr_rccl_library(void);      /* what was loaded, or why nothing was */
/* The library keeps the device and pinned-host blocks its contexts free in a process-wide cache (by device and size class) and
 * serves later allocations from it: a context's ~60 allocations cost 0.6-0.7 ms of a registration's first pass, and every free is a
 * device-wide synchronisation.  mvr_pool_trim gives all idle blocks back to the runtime and returns the bytes freed; stats (may be
 * NULL) receives {bytes still cached, requests served from the cache, requests that went to the runtime}.  Environment: MVR_POOL=0
 * switches the cache off, MVR_POOL_CAP_MB (default 16384) bounds what it holds. */
unsigned long long mvr_pool_trim(unsigned long long stats[3]);
/* the partition: edge_queries[e] = source points of edge e; rank's ranges (edge, first query, count), at most ne of them */
int  mvr_ring_segments(int ne, const size_t *edge_queries, int world, int rank, int *seg_edge, size_t *seg_begin, size_t *seg_count, int *n_seg);
/* arguments as mvr_ring_run; every rank passes the same poses in and gets the same poses out.  timing_ms = {enqueue,
 * wait for the GPU incl. the all-reduce, host solve}, summed over the passes.  A rank whose local work fails in a pass
 * reports it THROUGH that pass's all-reduce (a status row of the table), so all ranks return from the same pass -- the
 * failing rank with its own status, its peers with MVR_E_RCCL; a rank whose peers never arrive gives up after
 * "wait_timeout_ms" (mvr_ctx_tune, default 60 000), aborts the communicator (ncclCommAbort) and returns MVR_E_RCCL
 * (the context then refuses the multi-GPU entry points until mvr_ctx_comm_destroy + a new communicator).  The replicated
 * solve relies on RCCL's all-reduce handing every rank the SAME bits (one reduction order per element, whatever the
 * algorithm: ring and tree both reduce an element once and broadcast the result). */
int  mvr_ring_run_sharded(mvr_ctx *ctx, int n_steps, int n_views, const int *posed_slots, const int *raw_slots, int ne,
                          const int *edge_src, const int *edge_tgt, double max_dist, int reciprocal, int fma, const double origin[3],
                          int lum_iterations, double *poses, double *lum_pose, float *pair_T, double *pair_n, double *pair_mse,
                          int *lum_iters, double *rows, double *timing_ms);
/* one rank's half of ONE pass, for launchers that reduce the table themselves (MPI, a test): pose what `rank` of `world`
 * needs and return ITS rows of the edge table (zero rows for edges it does not touch; rows of a split edge are partial
 * sums) on the host.  The sum over the ranks' tables, fed to mvr_ring_host_step, is the pass. */
int  mvr_ring_rows_sharded(mvr_ctx *ctx, int rank, int world, int n_views, const int *posed_slots, const int *raw_slots, int ne,
                           const int *edge_src, const int *edge_tgt, double max_dist, int reciprocal, int fma, const double origin[3],
                           const double *poses, double *rows);
/* PROJECTION of one rank's share on ONE GPU (measurement aid, tools/rank_share_bench.py; no reference counterpart): after
 * mvr_ctx_project(ctx, world, rank, peer_rows, ne) mvr_ring_run_sharded plans and runs as `rank` of `world` -- its share of the
 * queries of registrator.cpp:640-651's edges, the collective of the context's communicator (a world of one) really issued --
 * and adds peer_rows ([ne][32], what the absent ranks would contribute: the sum of their mvr_ring_rows_sharded tables at the
 * poses the run starts from) to the table behind the all-reduce, so that the solve sees a whole table.  What it times is a
 * rank's critical path (its chain, the collective's launch, the replicated solve), NOT the fabric.  world <= 1: off. */
int  mvr_ctx_project(mvr_ctx *ctx, int world, int rank, const double *peer_rows, int ne);
/* (b) ONE process, all GPUs: n_dev contexts (device_ids NULL: 0 .. n_dev-1) + ncclCommInitAll;
 *     mvr_world_ring_run drives one host thread per device through mvr_ring_run_sharded and checks that every rank
 *     arrived at bit-identical poses.  mvr_world_upload puts a cloud into the same slot of every rank. */
typedef struct mvr_world mvr_world;
int  mvr_world_create(mvr_world **w, int n_dev, const int *device_ids);
int  mvr_world_destroy(mvr_world *w);
int  mvr_world_size(const mvr_world *w);
mvr_ctx *mvr_world_ctx(mvr_world *w, int rank);
const char *mvr_world_last_error(const mvr_world *w);
int  mvr_world_upload(mvr_world *w, int slot, const float *xyz, size_t n, size_t stride_bytes);
int  mvr_world_ring_run(mvr_world *w, int n_steps, int n_views, const int *posed_slots, const int *raw_slots, int ne, const int *edge_src,
                        const int *edge_tgt, double max_dist, int reciprocal, int fma, const double origin[3], int lum_iterations,
                        double *poses, double *lum_pose, float *pair_T, double *pair_n, double *pair_mse, int *lum_iters, double *rows,
                        double *timing_ms);
/* pcl::getTransformation(x,y,z,roll,pitch,yaw) -> column-major 4x4. */
void mvr_pose_to_mat4(const double pose[6], double T[16]);

/* ---- surface reconstruction (EXTENSION: pcl::MarchingCubesHoppe) -----------------------------------------------------------
 * The triangle mesh of a cloud that carries oriented normals: a lattice over the cloud's box, at every lattice vertex the signed
 * distance to the tangent plane of the nearest point, marching cubes over the lattice.  PCL was not at hand and the reference pins
 * no version; the rules restate pcl/surface/impl/marching_cubes.hpp and marching_cubes_hoppe.hpp (1.8 and later) as published:
 * PARITY WITH PCL UNPINNED.
 *  M1. Input: the cloud in `slot` with its normals.  A slot without normals is MVR_E_ARG before any GPU work; an empty slot is
 *      MVR_OK with zero triangles (grid_out, when given, is filled with NaN).
 *  M2. Box: lower / upper = the f32 componentwise min / max over the FINITE points (the library's rule; N5 applies), then
 *      ext = (0.5f * percentage_extend_grid) * (upper - lower), lower -= ext, upper += ext.  Every operation is rounded to f32 and
 *      no fma is used anywhere in M2-M8.
 *  M3. Voxel size: size = (upper - lower) / (float)res per axis -- by res, not res - 1: the lattice stops one voxel short of
 *      upper (PCL's behaviour, and why callers extend the grid).
 *  M4. Lattice vertex (x, y, z), 0 <= x < res_x ..., lies at v = lower + size * (float)i per axis (the multiply, then the add);
 *      its value is grid[x * res_y * res_z + y * res_z + z].
 *  M5. Value: with (j, d2) = mvr_nn's answer for v in the slot (the library's f32 d2, fma_dist as everywhere, ties to the lowest
 *      index, N1 for non-finite points) the value is NaN when there is no finite point; when dist_ignore > 0 and not
 *      d2 < dist_ignore (the SQUARED distance against dist_ignore: PCL's quirk, kept); when n_j.x is NaN; when the f32 norm
 *      sqrt((nx*nx + ny*ny) + nz*nz) of n_j is not > 0.5f.  Otherwise it is (n.x * dx + n.y * dy) + n.z * dz with d = v - p_j.
 *  M6. Cells (x, y, z), every index below res - 1, in x-major, z-fastest order.  Corners 0..7 at the offsets (0,0,0) (1,0,0)
 *      (1,0,1) (0,0,1) (0,1,0) (1,1,0) (1,1,1) (0,1,1).  A cell with a NaN corner emits nothing; cube |= 1 << i when
 *      value[i] < iso_level.
 *  M7. Corner positions: c = lower + size * index per axis; a corner is c plus size on the axes its offset is 1 on (one add).
 *  M8. Edges 0..11 join the corners 0-1 1-2 2-3 3-0 4-5 5-6 6-7 7-4 0-4 1-5 2-6 3-7.  Edge a-b gives
 *      mu = (iso - va) / (vb - va) and p = pa + mu * (pb - pa) on all three axes, always in that direction: neighbouring cells
 *      compute a shared edge in opposite directions and may differ in the last bit (PCL's behaviour, kept).
 *  M9. Output: the triangles of a cell in the case table's order, cells in M6's order; 3 * T vertices (xyz f32), polygon t is
 *      (3t, 3t + 1, 3t + 2).  A second run gives the same bits; the result depends neither on the resolution of the slot's grid
 *      nor on a tune key ("mc_route" included).
 * M10. Case tables: Lorensen / Bourke's edgeTable[256] and triTable[256][16], which PCL carries verbatim, written out once in
 *      csrc/mvr_mc_tables.h; mvr_mc_case hands a row to the host (what the tests and the numpy reference read).
 * M11. Sizing (the pattern of RS7): *n_triangles is written by every call that gets as far as the count (64-bit);
 *      vertices == NULL is a count-only call (*n_vertices = 3 T); capacity_triangles < T returns MVR_E_ARG with the counts
 *      written and nothing else.  grid_out: optional host array of res_x * res_y * res_z floats that receives the values.
 * M12. MVR_E_ARG before any GPU work, nothing written: a NULL ctx or params, a bad slot, a res below 2, res_x * res_y * res_z
 *      above 2^27, a non-finite iso_level or percentage_extend_grid, a negative percentage_extend_grid, a NaN dist_ignore
 *      (dist_ignore <= 0: no limit; PCL's default is -1), weld with vertices but without indices.
 * M13. Weld (EXTENSION, weld = 1): soup vertices on the same lattice edge become one; the key is 3 * (the 1-D index of M4 of the
 *      edge's lower vertex) + axis, not coordinates.  A welded vertex takes the position computed by the first soup corner that
 *      uses it; welded vertices are numbered in order of first use; polygons keep M9's order with the new indices; a triangle
 *      whose three indices are not all different is kept.  `vertices` then receives the n_vertices welded positions (it still
 *      needs room for 3 * capacity_triangles) and `indices` 3 * T u32.  Weld needs 3 * T < 2^31, else MVR_E_ARG after the count.
 * M14. Neither the slot nor its normals are modified (the slot gets its own-coordinates grid as in mvr_knn).
 * M15. An axis with upper == lower has size 0: M3-M8 literally, every vertex at the same position on that axis.
 * The search: tune key "mc_route" 0 (default) takes the walk of the cloud's own grid with a one-entry list that starts at the cap
 * when dist_ignore > 0, and otherwise the culled search behind mvr_nn over the lattice as query sets of at most 2^23 vertices
 * (a cloud that holds a non-finite point, for which that search has no rule, and a context in brute-force mode take the tiled
 * exact search in launches of at most 2^38 point pairs); 1 / 2 / 3 force the walk / the culled / the tiled search.  All give
 * mvr_nn's (j, d2) wherever the value is not NaN.  HAZARD: "mc_route" 1 WITHOUT a cap sends unbounded queries through the shell
 * walk -- exact, but a vertex far from the surface looks up millions of cells; it is there for the tests.  mvr_ctx_stat
 * "mc_route_used", and with tune "mc_clock" = 1 "mc_search_ms" / "mc_values_ms" / "mc_classify_ms" / "mc_emit_ms" /
 * "mc_weld_ms" / "mc_copy_ms". */
#define MVR_MC_MAX_VERTICES (1ull << 27)   /* M12: the most lattice vertices of one call */
typedef struct {
  int   res[3];                  /* setGridResolution: lattice vertices per axis, >= 2                 */
  float iso_level;               /* setIsoLevel                                                        */
  float percentage_extend_grid;  /* setPercentageExtendGrid: finite, >= 0                              */
  float dist_ignore;             /* setDistanceIgnore: <= 0 no limit; compared with the SQUARED distance */
  int   weld;                    /* EXTENSION (M13)                                                    */
  int   fma_dist;
} mvr_mc_params;
void mvr_mc_default_params(mvr_mc_params *p);   /* PCL's: 32, 32, 32, 0, 0, -1; weld 0, fma_dist 0 */
/* row `cube` (0..255) of the case tables: *edges = edgeTable[cube], tri = triTable[cube]; host only, no GPU */
int  mvr_mc_case(int cube, uint16_t *edges, int8_t tri[16]);
int  mvr_cloud_marching_cubes_hoppe(mvr_ctx *ctx, int slot, const mvr_mc_params *p, float *grid_out /* or NULL */,
                                    float *vertices /* 9 * capacity_triangles floats, or NULL */, size_t capacity_triangles,
                                    uint32_t *indices /* weld only: 3 * capacity_triangles */, uint64_t *n_triangles,
                                    uint64_t *n_vertices);

/* ---- turntable prior (PointCloud::initRotation point_cloud.cpp:400-413,
 *      Registrator::getRotationMatrix registrator.cpp:331-342) --------------- */
double mvr_turntable_angle(int view, int n_views);
/* Registrator::refineAxis (registrator.cpp:402-455, with math_solvers::least_squares, math_solvers.cpp:12-38): the
 * turntable axis and pivot that best explain the poses of the n REGISTERED views (poses: n x 16, column-major,
 * column-vector convention).  Axis: least squares of (R_i - I) x = 0 with the row u + v + w = 1, normalised; pivot:
 * least squares of (R_i - I) p = -t_i with the row p_y = pivot_y (the current pivot's y).  Results are floats, as the
 * reference's osg::Vec3.  MVR_E_ARG for n <= 0, MVR_E_SINGULAR for a rank-deficient system (outputs untouched). */
int    mvr_refine_axis(int n, const double *poses, float pivot_y, float axis_out[3], float pivot_out[3]);
void   mvr_axis_rotation(const double pivot[3], const double axis[3], double angle, double T[16]);
void   mvr_mat4d_mul(const double A[16], const double B[16], double C[16]);
void   mvr_mat4f_mul(const float A[16], const float B[16], float C[16]);

/* ---- instrumentation --------------------------------------------------------- */
/* per-kernel-family device time measured with HIP events on the ctx stream.
 * family: 0 = nn (brute-force NN, fwd + reciprocal), 1 = reductions (K5/K6/K8),
 * 2 = transform/copy, 3 = glue (mark/compact/weights). */
enum { MVR_K_NN = 0, MVR_K_REDUCE = 1, MVR_K_XFORM = 2, MVR_K_GLUE = 3,
       MVR_K_NN_GRID = 4,   /* the grid search of the fused pass: one thread per bounded query (work = point-pair evaluations) */
       MVR_K_NN_WIDE = 5,   /* its stragglers: wide bounded queries (a wave each) and flagged query sets (culled kernel over a set list) */
       MVR_K_COUNT = 6 };
/* knobs of the exact NN search.  "nn_mode": 1 (default) = spatially culled
 * kernel, 0 = brute-force kernel (also MVR_NN_MODE in the environment);
 * brute-force launch shape: "nn_q" (queries per lane: 2,4,6,8), "nn_sub"
 * (min-tracking sub-tile: 16,32,64), "nn_blocks_per_cu" (1..5); culled kernel:
 * "cull_q" (64-query groups per set: 1,2; 0 = auto), "cull_w" (waves sharing one
 * query set: 1,2,4; 0 = by launch size; also MVR_CULL_W); "pair_fused" (1, default: in culled mode
 * mvr_pair_moments2_batch runs every stage of all pairs as ONE launch; 0: one pair per worker stream;
 * also MVR_PAIR_FUSED), "pair_groups" (1..8, default 2: the fused pass runs its pairs in that many groups on
 * concurrent streams -- when there are at least four pairs per group -- so one group's small kernels overlap
 * another's searches; also MVR_PAIR_GROUPS),
 * "pair_streams" (worker streams, 1..16; also MVR_PAIR_STREAMS); "posed_refresh" (1, default: in culled mode
 * mvr_cloud_transform_batch also refreshes the index of the posed copies, from the sources' sorted copies;
 * 0: at the first search, by a gather; also MVR_POSED_REFRESH); "cull_slices" (1, 2, 4, 8; 0 = auto: a fused
 * launch deals each pair's query sets to the XCDs in that many interleaved slices, so that a pair's target is read
 * through that many of the eight L2s instead of all of them; 8 = every XCD visits every pair; also MVR_CULL_SLICES);
 * "seed_forward" (1, default: when a fused pass searches the very same point sets as the previous one on this context,
 * every forward search starts from the distance of its previous match; also MVR_SEED_FORWARD);
 * "ring_search" (1, default: in a fused pass every query that HAS a bound -- a forward search seeded by its previous
 * match, every reverse search -- walks a pose-invariant uniform grid over the target, one thread per query; 0: the
 * culled kernel answers everything; also MVR_RING_SEARCH), with its knobs "grid_cell_points" (points per occupied
 * cell the cell edge aims at, default 4; applies to grids built afterwards), "grid_light_rows" (rows of cells a thread
 * walks itself, default 24; wider balls leave the thread-per-query walk; "grid_light_rows_lone", default 12: the same in a
 * launch of one pair), "grid_wide" (1, default: a wide BOUNDED query
 * gets a wave of its own; 0: flagged for the culled kernel), "grid_cluster" (a wave of the walk with at least this many
 * wide queries hands them all to the culled kernel, default 8; 65: never), "grid_sets" (1, default: the 64-query
 * sets that hold a flagged query are answered a block per set over the grid while a set's union of balls is a few hundred
 * rows of cells; 2: always; 0: by the culled kernel over the set list), "grid_tail" (1, default: that launch and the
 * wave-per-query launch of a forward pass are one launch), "cull_list" (1, default: the culled kernel
 * visits only the query sets the walk listed; 0: a block per set), "cull_list_w" (waves per listed set: 1, 2, 4),
 * "grid_wide_waves" (waves per CU of the wave-per-query
 * launch), "fused_mark" (1, default: the forward searches record the start bounds of the reverse searches themselves when
 * they are the grid walk; 2: always; 0: never -- a separate launch re-reads the keys), "grid_debug" (1: every pass prints how its queries split; synchronises);
 * "pipeline" (1, default: mvr_ring_run / mvr_ring_run_sharded enqueue pass k+1's whole launch chain while pass k runs,
 * behind a hipStreamWaitValue32 gate the host opens after its solve, the poses reaching the kernels through a device table,
 * once a pass has run without allocating or waiting; 0: every pass is enqueued after the previous solve; also MVR_PIPELINE);
 * "grid_probe" (1, default: a query of the grid walk whose ball is wide first looks into the 2 x 2 x 2 cells nearest to it -- a
 * point found there is a tighter, valid bound; what a pass after a large motion needs; 0: off), "grid_probe_rows" (the probe is
 * made for balls of more than this many rows of cells, default 12, at most "grid_light_rows"; a probed query whose new ball lies inside the
 * probed cells is answered by the probe alone);
 * "lazy_super" (1, default: a posing launch that also writes a view's grid-ordered coordinates leaves its super boxes -- read by
 * the culled kernel alone -- to the first culled launch that follows, if any; 0: refreshed by every posing launch);
 * the aligns of the sequential mode: "seq_search" (mvr_icp_align of a posed scan: the forward search is the culled kernel's;
 * 1, default: the reverse searches walk the source scan's cell grid; 0: the culled kernel both ways),
 * "seq_cell_points" (points per occupied cell that the grid of a cloud over its own coordinates aims at -- the grid of the
 * k-NN, outlier, MLS, FPFH and pose-score searches; default 4), "seq_seed" (1, default: an align's forward searches start from the distance, now, of the point
 * each query matched when the same scan was last aligned on this context -- the sweeps of registrationICP, the rounds of
 * AutoReg; 0: off, and what the aligns so far have left is forgotten), "align_spin" (1, default: the last sums launch of a
 * point-to-point iteration stores the iteration's row into mapped pinned memory itself and the host spins on a sequence word;
 * 0: a copy behind the launch and hipStreamSynchronize), "seq_rider" (1, default: mvr_seq_run has the launch that poses the next
 * source refresh the grown model's index tail on the way; 0: a launch of its own inside the align), "reduce_rows" (blocks, = partial rows, per pair of the launches that carry the 29 raw sums;
 * 0, default: a quarter of the compute units, at least 32 -- the sums are added in an order that depends on it, so two runs
 * compare bit for bit only at the same value);
 * multi-GPU: "wait_timeout_ms" (how long a rank waits for a pass that contains a collective before it aborts its
 * communicator), and the test hooks "inject_fail_pass" / "inject_stall_pass" (the k-th sharded pass or iteration from now:
 * this rank's local work fails / its stream stalls in front of the collective as if a peer never arrived; -1: off).
 * Round 4: "grid_stage" (the staged walk: a wave of the grid walk copies the cells its lanes want into LDS -- LDS-DMA loads -- and
 * walks them there -- the two waves of a block one region together; 2, default: every walk launch; 1: only the launches over a scan's
 * own query order, i.e. the forward searches; 0: off; also MVR_GRID_STAGE), "grid_stage_stat" (1: counters of the staged walk's waves by outcome, read with
 * mvr_ctx_stat "stage_staged" / "stage_rows" / "stage_width" / "stage_points"), "grid_index" (a grid's cell-start table, for grids
 * built from then on: 2, default = dense, built through the compact form and expanded; 1 = compact: a directory of 32-cell segments
 * + records of the occupied ones, a tenth of the bytes, walks 8-11 % slower; any other value: MVR_E_ARG; also MVR_GRID_INDEX),
 * "order_batch" (1, default: the orderings several point sets need are built in one composite sort; 0: one after the other -- the
 * same permutations), "pipeline_multi_rank" (1: passes with a collective over more than one rank may be queued ahead of their poses
 * too; 0, default, until a recorded two-GPU run);
 * feature matching and pose scoring: "feat_split" (blocks the target of mvr_feature_knn is split over, 1..64; 0, default: by the
 * launch size), "score_chunk" (poses per launch of mvr_pose_scores, default 256); "pfh_stage" (mvr_cloud_pfh: the neighbourhood
 * size above which a query takes the tiled path, MVR_MAX_KNN..MVR_PFH_STAGE, default MVR_PFH_STAGE); "radius_stage"
 * (mvr_radius_search: the row length above which a row takes the long-row path, MVR_MAX_KNN..MVR_RADIUS_STAGE, default
 * MVR_RADIUS_STAGE); "at_sort" (the *_at entries: 1, default, sorts the queries by the cell of the surface's grid they fall in;
 * 0 takes them in the order given; no result depends on it), "at_clock" (1: mvr_cloud_fpfh_at records an event on its stream
 * around each of its four stages, created and destroyed per call, for the "fpfh_at_*_ms" stats; 0, default: none);
 * plane segmentation: "sac_chunk" (attempts generated and scored per chunk, 1..256; 0, default: 64 for the first chunk of a
 * call and 256 from then on);
 * the sample-consensus rejector: "rej_sac_chunk" (attempts generated and scored per chunk, 1..256; 0, default: 64 for the first
 * chunk of a stage and 256 from then on -- measured, profiles/reject_sac_bench.json);
 * marching cubes: "mc_route" (the search behind the lattice values: 0, default, by dist_ignore; 1 the own-grid walk -- without a
 * dist_ignore it is slow beyond use on anything but a test cloud --; 2 the culled search; 3 the tiled exact search; see
 * mvr_cloud_marching_cubes_hoppe), "mc_clock" (1: the call waits after each stage and records its wall milliseconds for the
 * "mc_*_ms" stats; 0, default: no waits).
 * Results never depend on them. */
int  mvr_ctx_tune(mvr_ctx *ctx, const char *key, int value);
/* wall milliseconds of every pass of the LAST mvr_ring_run / mvr_ring_run_sharded on this context (from the end of the
 * previous pass's solve to the end of this one's; the first from the start of the call): what the first passes of a
 * registration cost (orderings, grids) beside the steady state.  *n = passes logged (may exceed cap). */
int  mvr_ctx_pass_log(mvr_ctx *ctx, double *ms, int cap, int *n);
/* counters of the context, by name: "piped_passes" (passes of mvr_ring_run / mvr_ring_run_sharded whose launch chain was
 * enqueued ahead of their poses, see "pipeline"), "fused_passes" (fused pair batches run so far), "blocking_events"
 * (times the library waited for its stream or re-allocated a buffer: a pass without any is in steady state),
 * "prerej_match_ms" / "prerej_hypotheses_ms" / "prerej_score_ms" (wall milliseconds of the last mvr_align_prerejective by phase),
 * "pfh_stage" (the tune key's value), "pfh_tiled_queries" / "pfh_pairs" (of the last mvr_cloud_pfh: see there),
 * "at_sort" (the tune key's value), "fpfh_at_marked" (of the last mvr_cloud_fpfh_at: the surface points whose SPFH row was
 * computed), "fpfh_at_mark_ms" / "fpfh_at_select_ms" / "fpfh_at_spfh_ms" / "fpfh_at_weight_ms" (device milliseconds of its stages --
 * the marking walk, the flagged selection with the read-back of its count, the SPFH rows, the weighting -- when the tune key
 * "at_clock" was 1 during the call, else 0),
 * "radius_stage" (the tune key's value), "radius_long_rows" (of the last mvr_radius_search: rows on the long-row path),
 * "radius_count_ms" / "radius_fill_ms" / "radius_copy_ms" (wall milliseconds of the last mvr_radius_search by phase: the count up to
 * the read-back of the total; the fill and the ordering of the rows, with the copy of the offsets; the copies of idx / d2 to the host) */
int  mvr_ctx_stat(mvr_ctx *ctx, const char *key, double *value);
/* diagnostics: the ordering of the cloud in `slot` (sorted position -> original index); *n = its length (0: none yet) */
int  mvr_debug_order(mvr_ctx *ctx, int slot, uint32_t *perm, size_t cap, size_t *n);
/* diagnostics of the culled kernel: {pair evaluations of the last launch,
 * running total, max tiles processed by one wave, max tiles tested by one wave} */
int  mvr_debug_counters(mvr_ctx *ctx, uint64_t out[4], int reset);
/* per-launch HIP-event timing: 0 off, 1 all kernel families, 2 the NN search kernels only */
int  mvr_prof_enable(mvr_ctx *ctx, int on);
int  mvr_prof_reset(mvr_ctx *ctx);
/* launches, total ms, point-pair evals (nn families) / bytes (others) */
int  mvr_prof_get(mvr_ctx *ctx, int family, uint64_t *launches, double *ms, double *work);

/* ---- synthetic turntable scans (host only, no GPU needed) --------- */
typedef struct {
  int      n_views;        /* V: views at 2*pi/V                            */
  uint64_t seed;           /* base seed; view v uses seed + v               */
  double   noise_sigma;    /* along-normal noise, mm                        */
  double   pivot[3];       /* true turntable pivot (point_cloud.cpp:102)    */
  double   axis[3];        /* true turntable axis  (point_cloud.cpp:103)    */
} mvr_synth_params;
void mvr_synth_default(mvr_synth_params *p, int n_views, int config_id);
/* fills xyzw (n*4 floats, w=1) and, if non-NULL, normals (n*4 floats, w=0) of
 * the scan of `view`: object rotated by +view*2pi/V about (pivot, axis). */
int  mvr_synth_view(const mvr_synth_params *p, int view, size_t n, float *xyzw, float *normals);
/* the mis-calibrated prior handed to initRotation: pivot + (1.5,-1,2) mm and
 * the axis tilted by 0.5 deg about x. */
void mvr_synth_prior(const mvr_synth_params *p, double pivot[3], double axis[3]);

#ifdef __cplusplus
}
#endif
#endif /* MVR_HIP_H */
