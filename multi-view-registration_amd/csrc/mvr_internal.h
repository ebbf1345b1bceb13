// csrc/mvr_internal.h -- shared declarations of libmvr_hip.so (not installed).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <map>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "mvr_hip.h"

// ---- every device / pinned-host allocation of the library goes through a process-wide cache of freed blocks (mvr_pool.cpp): the names
// of the runtime's four calls are redirected HERE, after the runtime's and hipCUB's own headers (a translation unit that uses hipCUB
// includes it before this file), so that no call site has to know
namespace mvr {
hipError_t pool_malloc(void **p, size_t bytes);
hipError_t pool_free(void *p);
hipError_t pool_host_malloc(void **p, size_t bytes, unsigned flags);
hipError_t pool_host_free(void *p);
template <class T> inline hipError_t pool_malloc_t(T **p, size_t bytes) { return pool_malloc(reinterpret_cast<void **>(p), bytes); }
template <class T> inline hipError_t pool_host_malloc_t(T **p, size_t bytes, unsigned flags = 0) { return pool_host_malloc(reinterpret_cast<void **>(p), bytes, flags); }
template <class T> inline hipError_t pool_free_t(T *p) { return pool_free(const_cast<void *>(static_cast<const void *>(p))); }
template <class T> inline hipError_t pool_host_free_t(T *p) { return pool_host_free(const_cast<void *>(static_cast<const void *>(p))); }
}  // namespace mvr
#define hipMalloc(p, n) ::mvr::pool_malloc_t((p), (n))
#define hipFree(p) ::mvr::pool_free_t(p)
#define hipHostMalloc(...) ::mvr::pool_host_malloc_t(__VA_ARGS__)
#define hipHostFree(p) ::mvr::pool_host_free_t(p)

namespace mvr {

// ---- device data layout ------------------------------------------------------
// Morton ordering of one point SET, shared by every cloud that holds that set
// (a posed copy of a scan keeps the scan's ordering: rigid motion does not
// change which points are neighbours).
// Buffers of dropped orderings, kept for the next one: a target that grows by one scan per align gets a new
// ordering every time, and hipFree + hipMalloc of its two index arrays (a device-wide synchronisation each) cost
// more host time than the whole align took on the GPU (0.45 of 1.0 ms, rocprofv3 timeline of the sequential mode).
// One pool per context: a recycled buffer is next written by a kernel on the same stream, after its last reader.
struct OrderPool {
  struct Buf { uint32_t *p; size_t bytes; };
  std::vector<Buf> free;
  bool closed = false;
  uint32_t *take(size_t bytes, size_t *got);
  void give(uint32_t *p, size_t bytes);
  void close();
  ~OrderPool() { close(); }
};
struct Order {
  uint32_t *perm = nullptr;   // sorted position -> original index
  uint32_t *inv = nullptr;    // original index  -> sorted position
  size_t n = 0;
  size_t perm_bytes = 0, inv_bytes = 0;
  std::shared_ptr<OrderPool> pool;
  std::shared_ptr<char> arena;         // set: perm / inv are carved out of this block, shared with the other orderings of one batched build (freed with the last of them)
  ~Order();
};

// Uniform grid over a point SET in its CANONICAL coordinates (the coordinates it was uploaded with): like the ordering
// it belongs to the set, is built once per scan and shared by every posed copy -- a rigid motion moves the points, not
// their cells.  A search in a posed copy maps the query into the canonical frame (inverse of the copy's pose), walks the
// cells its search ball overlaps, and evaluates the candidates in the POSED frame (same float arithmetic as every other
// search kernel: bit-identical distances).  See mvr_grid.hip.
constexpr int kDtShift = 1;            // a grid's distance map is kept per cube of 2 x 2 x 2 cells: an eighth of the bytes and of the build
struct CellGrid {
  size_t n = 0;
  float lo[3] = {0, 0, 0};
  float h = 1.f, inv_h = 1.f;            // cell edge
  int dim[3] = {1, 1, 1};                // cells per axis; cell id = (z * dim[1] + y) * dim[0] + x
  // Where a cell's points begin, in ONE of two forms (the tune key grid_index; both built by build_compact_grids, same walks' results):
  // DENSE (the default): start[c] = first grid position of cell c (points sorted by cell id), start[cells] = n, kStartPad more
  // entries of n behind it; dir and recs are null.
  // COMPACT (`start` is then null): the cell ids are cut into segments of 32 consecutive ids; an occupied segment has a record of
  // its 32 starts in recs[], an empty one -- all its cells begin at the same position -- is the directory entry itself:
  // dir[seg] = slot | 0x80000000 or that position.  A 200k-point scan occupies ~1/20 of its 375k segments: 1.5 MB of directory +
  // 2.5 MB of records instead of 48 MB of which a walk touched a 128-byte line per row for three entries.
  uint32_t *start = nullptr;
  uint32_t *dir = nullptr, *recs = nullptr;
  uint32_t nseg = 0;
  int dtdim[3] = {1, 1, 1};              // the distance map's dimensions: one byte per cube of 2^kDtShift cells per axis
  uint32_t *gperm = nullptr;             // [n] grid position -> original index
  float4 *graw = nullptr;                // [n] canonical coordinates in grid order, w = bits(original index)
  uint32_t *g2h = nullptr;               // [n] grid position -> position in the set's Hilbert ordering (what the fused pass's keys carry)
  uint32_t *h2g = nullptr;               // [n] its inverse: where a seed (a Hilbert position) sits in grid order -- the seed's coordinates then come from the array the walk reads anyway
  char *block = nullptr;                 // the ONE device allocation the arrays below are carved out of
  hipEvent_t ready = nullptr;            // set when the grid was built on the context's side stream: recorded behind its last build kernel
  bool ready_waited = false;             // ... and the context's main stream has been made to wait for it
  uint8_t *dt = nullptr;                 // [cubes] Chebyshev distance, in cubes, to the nearest occupied cube (0 = occupied, 255 = farther than dt_steps): "is there any point near here at all" in ONE byte
  int dt_steps = 0;                      // dilation steps dt was built with: 255 means "farther than dt_steps cubes"
  const Order *built_for = nullptr;      // the ordering g2h refers to
  ~CellGrid();
};

// A cloud is an array of float4 {x,y,z,1}: the same 16-byte record as
// pcl::PointXYZ (mvr/include/types.h:14), so a host upload is one memcpy and
// every lane moves one point with a single 16-byte access (dwordx4).
// For the culled search it also carries a Morton-ordered copy (w = bits of the
// original index) and one AABB per 256-point tile of that copy.
// A cloud may be a SHARD of a larger (distributed) cloud: segment k says that local points
// [local_begin, local_begin + count) are global points [global_begin, global_begin + count).
// No segments = the cloud is its own global numbering.
struct Seg { uint32_t local_begin, count, global_begin; };
constexpr int kMaxSegs = 64;
struct SegTable { uint32_t n; uint32_t lb[kMaxSegs], cnt[kMaxSegs], gb[kMaxSegs]; };

struct Mat44d { double m[16]; };
// pose-derived parameters of one posed cloud, in DEVICE memory: what the kernels of a pass that was enqueued before its
// poses were known read instead of by-value arguments (the pipelined ring run, mvr_ctx.hip)
struct PoseRec {
  Mat44d T;                 // the pose (column-major 4 x 4)
  double minv[12];          // its inverse affine map, row-major 3 x 4: posed frame -> canonical frame
  float stretch;            // bound of how much the inverse lengthens a distance (1 for a rigid pose)
};

struct Cloud {
  float4 *pts = nullptr;
  size_t n = 0;
  size_t cap = 0;
  uint64_t set_id = 0;                 // identity of the point set + its indexing
  std::shared_ptr<Order> order;        // null until first needed
  float4 *sorted = nullptr; size_t sorted_cap = 0;
  float4 *tlo = nullptr, *thi = nullptr; size_t tiles_cap = 0;
  float4 *cbox = nullptr;              // [tiles][4 cells][lo, hi]: AABBs of the 64-point cells of every tile
  float4 *sbox = nullptr;              // [ceil(tiles / 64)][lo, hi]: AABBs of 64 consecutive tiles
  bool super_stale = false;            // sbox[] was NOT refreshed with the tile boxes (a posed copy about to be searched over its grid): flush_super_boxes() before a culled launch
  bool coords_valid = false;           // sorted[] / tlo / thi / cbox match pts[]
  size_t fresh_tiles = 0;              // with !coords_valid: that many LEADING tiles of sorted[] / boxes are still current (a cloud that only grew at its end: mvr_cloud_append with an extended ordering); any other change of the coordinates resets it
  void stale_coords() { coords_valid = false; fresh_tiles = 0; gcoords_valid = false; mgrid_ok = false; sorted_stale = false; lean_raw = nullptr; }
  // optional unit normals {nx,ny,nz,0} (point-to-plane extension, K10)
  float4 *nrm = nullptr; size_t nrm_cap = 0;
  bool has_normals = false;
  std::vector<Seg> segs;               // global numbering of a shard (target sharding over ranks)
  // pose bookkeeping for the grid search: `canonical` = these ARE the set's upload coordinates; otherwise, when
  // pose_known, pts = pose * (canonical coordinates of the set) exactly as mvr_cloud_transform computes it
  bool canonical = false, pose_known = false;
  double pose_stretch = 1.0;             // with pose_known: an upper bound of how much the INVERSE pose can lengthen a distance (1 for a rigid pose; the poses of a long registration are products of float-rounded matrices and drift away from orthonormal)
  double pose[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  std::shared_ptr<CellGrid> grid;          // the set's grid (shared)
  float4 *gsorted = nullptr; size_t gsorted_cap = 0;      // posed coordinates in grid order, w = bits(original index)
  bool gcoords_valid = false;          // gsorted matches pts
  std::shared_ptr<CellGrid> mgrid;     // a grid over THESE coordinates (ensure_model_grid: what the k-NN, outlier, MLS, FPFH and pose-score walks search), valid while mgrid_ok
  bool mgrid_ok = false;
  // pipelined ring run (mvr_ctx.hip: ring_passes): where the kernels of a pass that is enqueued BEFORE its poses are known
  // find this posed copy's pose, inverse and stretch (device memory, filled by pose_prep_kernel once the host's solve has
  // released the pass); null outside such a run
  const struct PoseRec *pose_dev = nullptr;
  void forget_pose() { canonical = false; pose_known = false; pose_stretch = 1.0; grid.reset(); }
  float bbox[6] = {0, 0, 0, 0, 0, 0}; uint64_t bbox_set = 0;      // with bbox_set == set_id (and canonical): the bounding box of pts[], taken when the cloud was uploaded (the grid build then needs no round trip for it)
  bool pts_stale = false;              // pts[] were left out by the last (pipelined) pose of this cloud: sorted[] / gsorted[] are current, pts[] are written when the run leaves the pipe
  bool posed_by_table = false;         // ... and the last transform of this cloud did read it (its host-side pose is filled in when the run leaves the pipe)
  // the last (pipelined) pose of this cloud was LEAN: only gsorted[] and the device pose record were written.  sorted[] and the
  // boxes are NOT current although coords_valid says so -- the kernels of such a pass pose their queries themselves, from
  // lean_raw[] (the raw scan's Hilbert-ordered copy: same order, same w) and the record; whoever wants the arrays themselves
  // calls flush_lean_sorted() first (ensure_index / ensure_index_batch do), and the run writes them when it leaves the pipe
  bool sorted_stale = false;
  const float4 *lean_raw = nullptr;
};

constexpr uint32_t kNone = 0xFFFFFFFFu;      // "no neighbour" index
constexpr uint32_t kMarked = 0xFFFFFFFEu;    // slot[] state between CAS and list position

// NN key: (float bits of d2) << 32 | index.  d2 >= 0, so the unsigned order of
// the key is (d2, index) lexicographic: an integer min gives the nearest
// neighbour with ties resolved to the lowest index.
using nnkey_t = unsigned long long;
constexpr nnkey_t kKeyInit = ~0ull;

// brute-force NN tiling (see mvr_nn.hip)
constexpr int kNNThreads = 256;   // 4 waves
constexpr int kNNTile = 1024;     // target points per LDS tile (16 KB)
// Q (queries held in registers per lane) and SUB (sub-tile over which only
// min(d2) is tracked) are template parameters, chosen per ctx (nn_q, nn_sub).

// culled NN (see mvr_index.hip): tile of the Hilbert-ordered target cloud
constexpr int kCullTile = 256;
// its evaluation counters are sharded (one 128-byte line per shard) so that
// thousands of waves do not serialise on one address; region A = this launch,
// region B = {running total, max tiles per wave, max tiles tested} per shard
constexpr int kEvalShards = 64, kEvalStride = 16;
constexpr size_t kEvalRegion = (size_t)kEvalShards * kEvalStride;     // u64 per region
constexpr size_t kTraceBlocks = 4096, kTraceRec = 16;   // diagnostic builds (-DMVR_TRACE): per-block records of the last launch, after the two regions

// work = `work` unless `h_count` is set: then work = *h_count * per_count (the
// query count / evaluation count is only known on the device)
struct ProfRec { int family; hipEvent_t a, b; double work; const uint64_t *h_count; int n_shards; double per_count; };

// where the searches of one pair of the last fused batch left their keys (mvr_pair_batch_correspondences)
struct Ctx;
struct BatchPairRec { Ctx *w = nullptr; size_t off_s = 0, off_t = 0, qb = 0, qn = 0; int src = -1, dst = -1; double max2 = 0.0; int reciprocal = 0; unsigned long long src_set = 0, dst_set = 0; };

struct Ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  int n_cu = 0;
  struct Cloud *refresh_rider = nullptr;              // refresh_posed_batch: a cloud whose stale index is refreshed by the same launch (set around a call, never kept)
  int reduce_rows = 0;                                // blocks (= partial rows) per pair of the launches that carry 29 sums per lane; 0: a quarter of the CUs (at least 32)
  int clock_mhz = 0;
  std::string name;
  std::string last_error;
  Cloud slots[MVR_MAX_SLOTS + 2];          // +2 internal scratch clouds
  uint64_t next_set_id = 1;
  std::map<uint64_t, std::weak_ptr<Order> > orders;   // set_id -> ordering (shared between posed copies)
  std::map<uint64_t, std::weak_ptr<CellGrid> > grids;     // set_id -> uniform grid (shared between posed copies)
  int grid_probe = 1;                                 // grid search: a query whose ball is wide first looks into the 2 x 2 x 2 cells nearest to it -- a point found there is a tighter (valid) bound, and most wide balls of a pass after a large motion are loose bounds, not far neighbours (0: off)
  int grid_probe_rows = 12;                           // ... the probe is made for balls of more than this many rows of cells (<= grid_light_rows; the 2 x 2 x 2 cells are four rows)
  int grid_light_rows_lone = 12;                      // ... in a launch of ONE pair (measured on the sequential mode's reverse searches: 24 costs an align 8 us)
  int grid_light_rows = 24;                           // grid search (default = kGridLightRows): rows of cells a thread walks itself; wider balls leave for a wave of their own or for the culled kernel
  // mvr_icp_align of a posed scan remembers, per point set, where each query's match sat in the target (sorted position) and
  // starts the NEXT align of that scan from the distance of that point under the current coordinates: the sweeps of the sequential
  // mode (registrator.cpp:530-577, repeat_times of them) and the rounds of AutoReg align the same scans again and again against a
  // model that has barely moved.  Any target point gives a valid inclusive bound, so a stale seed costs time, never exactness.
  int seq_seed = 1;
  struct SeedBuf { uint32_t *d = nullptr; size_t n = 0, cap = 0; };
  std::unordered_map<unsigned long long, SeedBuf> seq_seeds;      // by the source's point-set id
  uint32_t *seed_bound = nullptr; size_t seed_bound_cap = 0;
  struct G2HJob { std::shared_ptr<CellGrid> grid; std::shared_ptr<Order> order; size_t n; };
  std::vector<G2HJob> g2h_todo;                       // grid_coords_prepare -> flush_g2h
  int unseeded_grid = 0;                              // 1: the forward searches of a fused pass WITHOUT seeds (a registration's first) walk the grid as well (probe, then the listed sets) instead of the culled kernel
  int seq_cell_points = 4;                            // points per occupied cell the grid of a cloud over its own coordinates aims at (every ensure_model_grid)
  int seq_search = 1;                                 // mvr_icp_align of a posed scan: the forward search is the culled kernel's; the REVERSE searches 1 (default) = walk the source scan's cell grid (compaction by the fused pass's kernels, no hipCUB), 0 = take the culled kernel too
  int ring_search = 1;                                // fused pass: 1 = seeded searches walk the uniform grid (thread per query), 0 = always the culled kernel
  std::shared_ptr<OrderPool> order_pool = std::make_shared<OrderPool>();
  // per-pair work buffers (grown on demand)
  nnkey_t *keys = nullptr;   size_t keys_cap = 0;     // [Ns] forward NN keys (by original source index)
  nnkey_t *rkeys = nullptr;  size_t rkeys_cap = 0;    // [Nt'] reverse NN keys (by list position)
  uint32_t *slot = nullptr;  size_t slot_cap = 0;     // [Nt] target -> list position
  uint32_t *list = nullptr;  size_t list_cap = 0;     // [Nt'] distinct matched targets
  int32_t *match = nullptr;  size_t match_cap = 0;    // [Ns] accepted match or -1
  uint8_t *flags = nullptr;  size_t flags_cap = 0;    // [Nt] matched-target flags (culled mode, sorted space)
  uint32_t *bound = nullptr; size_t bound_cap = 0;    // [Nt] start bounds of the reverse searches (culled mode, sorted space)
  uint32_t *count = nullptr;                          // device counter (list length)
  unsigned long long *evals = nullptr;                // device counter: pair evaluations of the culled kernel
  double *partials = nullptr; size_t partials_cap = 0;
  double *moments = nullptr;                          // device: 64 doubles
  double *h_moments = nullptr;                        // pinned host: 64 doubles
  // mvr_icp_align's one round trip per iteration: the last sums launch stores the iteration's 19 doubles into mapped pinned
  // memory itself and then a sequence word the host spins on (align_spin; a copy packet + hipStreamSynchronize cost ~25 us)
  double *h_align = nullptr, *d_align = nullptr;      // pinned host, 64 doubles + the word (at double 64), and the device's view of it
  uint32_t align_seq = 0;
  int align_spin = 1;
  // correspondence rejectors (mvr_reject.hip): the chain's device state -- kRejRowDoubles doubles of sums (raw moments at 0,
  // point-to-plane at 32), then the stage words, which one copy brings to rej_host together; then histogram and block counts
  double *rej_row = nullptr, *rej_host = nullptr;     // device, pinned host (the copied part only)
  nnkey_t *rej_win = nullptr; size_t rej_win_cap = 0; // ONE_TO_ONE: per target the smallest (d2 bits << 32 | query); all ~0 between calls
  bool rej_win_dirty = false;                         // ... unless a chain failed between marking and clearing: filled again before the next use
  // Generalized ICP (mvr_gicp.hip): the optimiser's state block (layout at kGicpStateDoubles below) and its pinned host copy
  double *gicp_state = nullptr, *gicp_host = nullptr;
  int seq_rider = 1;                                  // mvr_seq_run: the model's tail is refreshed by the launch that poses the next source
  // index-build scratch
  uint32_t *codes_a = nullptr, *codes_b = nullptr, *idx_a = nullptr; size_t sort_cap = 0;
  void *cub_tmp = nullptr; size_t cub_cap = 0;
  char *scratch = nullptr; size_t scratch_cap = 0;    // temporaries of the grid builds (grows, never shrinks)
  char *oscratch = nullptr; size_t oscratch_cap = 0;  // temporaries of a batched ordering build (its own buffer: the grid builds use `scratch` on the side stream meanwhile)
  int order_batch = 1;                                // 1 (default): the orderings a call needs for several point sets are built together (one sort); 0: one set after the other
  hipStream_t side_stream = nullptr;                  // set-up work that may overlap a pass (grid builds)
  hipEvent_t side_after = nullptr;                    // recorded on the main stream before the pass the side stream's work overlaps
  hipEvent_t scratch_event = nullptr; hipStream_t scratch_stream = nullptr;      // the last user of `scratch`
  float *bbox = nullptr;                              // device: 8 floats (lo xyz, hi xyz)
  // launch configuration (mvr_ctx_tune)
  int nn_q = 8, nn_sub = 32, nn_blocks_per_cu = 2;
  int nn_mode = 1;                                    // 0: brute force, 1: culled (exact, identical results)
  int cull_q = 0;                                     // culled kernel: queries per lane (0 = auto)
  int cull_w = 0;                                     // culled kernel: waves sharing one query set (1, 2, 4; 0 = by launch size)
  int cull_slices = 0;                                // culled kernel: interleaved slices a pair's query sets are dealt to the XCDs in (1, 2, 4, 8; 0 = 8 / gcd(pairs, 8))
  int seed_forward = 1;                               // fused pass: forward searches start from the previous pass's matches when the same pairs are searched again
  int fused_mark = 1;                                 // fused pass: the forward launches themselves record the matched targets' start bounds -- 1: when they are the grid walk, 2: always, 0: never (a separate launch re-reads the keys)
  bool marked_in_search = false;                      // ... what this pass does (decided with its forward launches)
  std::vector<BatchPairRec> last_batch;               // the pairs of the last fused mvr_pair_moments2_batch on this context
  unsigned long long fused_passes = 0;                // fused pair batches run on this context so far
  std::vector<unsigned long long> fused_sig;          // what the forward keys in bkeys[] belong to (point-set ids, ranges, offsets): the previous fused pass on this context
  int pair_streams = 6;                               // worker streams of mvr_pair_moments2_batch
  // workers: contexts with their own stream and work buffers that BORROW clouds of this
  // context (slots 0/1) so that independent scan pairs run concurrently on the GPU
  std::vector<Ctx *> workers;
  Ctx *parent = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  double *batch_table = nullptr; size_t batch_cap = 0;   // [pairs][32] staging of mvr_pair_moments2_batch
  // feature matching and pose scoring (mvr_feature.hip): blocks a target is split over (0: by the launch size) and poses per
  // scoring launch -- results never depend on either; wall milliseconds of the last mvr_align_prerejective by phase
  int feat_split = 0, score_chunk = 256;
  int pfh_stage = MVR_PFH_STAGE;                         // neighbours a PFH query stages in LDS; above it the tiled path (tune "pfh_stage")
  int radius_stage = MVR_RADIUS_STAGE;                   // neighbours a radius-search row stages (and orders) in LDS; above it the long-row path (tune "radius_stage")
  uint64_t radius_long_rows = 0;                         // of the last mvr_radius_search: rows on the long-row path
  double radius_ms[3] = {0.0, 0.0, 0.0};                 // ... and its wall milliseconds: the count (to the read-back of the total), the fill and ordering, the copies home
  // marching cubes (mvr_mc.hip): which search answers the lattice vertices (tune "mc_route": 0 = by dist_ignore, 1 = the walk of
  // the cloud's own grid, 2 = the culled search over slabs of the lattice, 3 = the tiled exact search of mvr_nn.hip; no result
  // depends on it), the route the last call took, whether the stages are timed (tune "mc_clock"), and their wall milliseconds:
  // search, values, classify + scan, emit, weld, copies home
  int mc_route = 0, mc_route_used = 0, mc_clock = 0;
  double mc_ms[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  uint64_t pfh_tiled = 0, pfh_pairs = 0;                 // of the last mvr_cloud_pfh: queries on the tiled path, pairs of all queries
  int at_sort = 1;                                       // the _at entries sort their queries by the surface's cells (tune "at_sort"); results never depend on it
  uint64_t fpfh_at_marked = 0;                           // of the last mvr_cloud_fpfh_at: surface points whose SPFH row was computed
  int at_clock = 0;                                      // tune "at_clock": mvr_cloud_fpfh_at times its stages with events on its stream ...
  float fpfh_at_ms[4] = {0.f, 0.f, 0.f, 0.f};            // ... mark, select (with the read-back of the count), SPFH, weight; 0 without the key
  double prerej_ms[3] = {0.0, 0.0, 0.0};                 // matching, hypothesis generation, scoring
  int rej_sac_chunk = 0;                                 // the sample-consensus rejector: attempts per chunk (0: 64 for a stage's first chunk, 256 from then on -- profiles/reject_sac_bench.json); results never depend on it
  mvr_rej_sac_result last_sac = {}; bool last_sac_set = false;      // the last sample-consensus stage that ran on this context (mvr_ctx_last_sample_consensus)
  int sac_chunk = 0;                                     // mvr_cloud_segment_plane: attempts per chunk (0: 64 for a call's first chunk, 256 from then on); results never depend on it
  char *dn_arena = nullptr; size_t dn_arena_cap = 0;     // scratch of mvr_cloud_denoise and mvr_cloud_voxel_grid (one buffer, carved per call)
  int ndt_dense_max = 1 << 24;                           // NDT: the largest lattice (voxels) that gets the dense voxel -> cell table; above it the kept keys are searched (same bits)
  uint32_t *ndt_table = nullptr; size_t ndt_table_cap = 0;      // that table
  double *h_table = nullptr; size_t h_table_cap = 0;     // pinned host memory the final kernels of mvr_ring_step write straight into (zero-copy)
  // workspace of the fused batch (culled mode): forward keys of all pairs, reverse keys + flags, per-pair partial rows
  nnkey_t *bkeys = nullptr; size_t bkeys_cap = 0;
  nnkey_t *brkeys = nullptr; size_t brkeys_cap = 0;
  uint32_t *bwide = nullptr; size_t bwide_cap = 0;       // [sources + targets of all pairs] grid search: ordinals of the wide bounded queries
  int grid_cell_points = 4;                              // points per occupied cell the grid's cell edge aims at (grids built from then on)
  int grid_index = 2;                                    // a grid's cell-start table (grids built from then on): 2 (default) = DENSE, built through the compact form (all scans sorted at once, distance map per 2 x 2 x 2 cells) and expanded; 1 = COMPACT (segment directory + records of the occupied segments: a tenth of the bytes, walks 8-11 % slower)
  // the STAGED walk (mvr_grid.hip): a wave of the one-lane-per-query walk copies the box of its lanes' cells into LDS with a few
  // coalesced loads and every lane walks its own cells there -- the walk is bound by the number of vector memory instructions a
  // wave issues, not by bytes.  0: the plain walk; 1 (default): launches over a scan's own query order (the forward searches); 2: every
  // launch, compacted query lists too (measured equal or slower there).  A lone pair's launch has its own switch.
  int grid_stage = 2, grid_stage_lone = 1;      // (2 since the two waves of a block stage one region together: the reverse launches' sparser queries fit it too)
  unsigned long long *stage_stat = nullptr;              // diagnostics (tune key grid_stage_stat = 1): device counters [64 shards][64] of the staged walk's waves: [1] staged, [2] too many rows, [3] too wide, [4] too many points
  int grid_cluster = 8;                                  // a wave of the grid search with at least this many wide queries hands them ALL to the culled kernel (65: never)
  int grid_wide_waves = 32;                              // waves per CU of the wave-per-query launch
  int grid_tail = 1;                                     // 1: the wave-per-query launch and the listed-sets launch of a forward pass are one launch
  int grid_sets = 1;                                     // the listed query sets of a seeded forward pass: 1 = over the grid (nn_grid_set_kernel) while a set's union of balls is a few hundred rows of cells, 2 = always over the grid, 0 = by the culled kernel over the set list
  int cull_list = 1;                                     // 1: the grid search lists the query sets it flags and the culled kernel walks that list (0: a block per set, most of which leave at once)
  uint32_t *bcull_sets = nullptr; size_t bcull_sets_cap = 0;
  int cull_list_w = 2;                                   // waves per query set of the set-list launch of the culled kernel (1, 2 or 4)
  int grid_debug = 0;                                    // 1: every fused pass prints how its queries split between the three searches (synchronises: diagnostics only)
  int grid_wide = 1;                                     // 1: wide BOUNDED queries of the grid search get a wave each (0: flagged for the culled kernel like the unbounded ones)
  uint32_t *bwide_count = nullptr;                       // [2 * kBatchPairs ...] their counts (zeroed by the pass's moments launch)
  uint8_t *bheavy = nullptr; size_t bheavy_cap = 0;      // [sources of all pairs] grid search: queries left to the culled kernel (wide balls)
  uint32_t *bbound = nullptr; size_t bbound_cap = 0;     // [targets of all pairs] bits of the forward d2 of a source that matched the target (~0: not matched)
  bool bbound_clean = false;                             // bbound[] is all ~0 (the moments launch of a pass restores what its forward launch marked)
  uint32_t *blist = nullptr; size_t blist_cap = 0;
  uint32_t *bslot = nullptr; size_t bslot_cap = 0;
  uint32_t *bchunks = nullptr; size_t bchunks_cap = 0;      // per-chunk counts / offsets, then one count per pair
  double *bpartials = nullptr; size_t bpartials_cap = 0;
  int inplace_ratio = 3;                              // culled reverse search in place (flags) when nt < ratio * queries, else compacted list
  int pair_fused = 1;                                 // culled mode: all pairs of a batch in one launch per stage (0: worker streams)
  int posed_refresh = 1;                              // mvr_cloud_transform_batch brings the posed copies' index up to date from the sources' sorted copies
  int pair_groups = 2;                                // fused pass: groups of pairs on concurrent streams (1: a single stream); measured on the 12-pair ring: 1.27 / 1.22 / 1.28 / 1.39 ms per step with 1 / 2 / 3 / 4
  // ---- pipelined ring run (ring_passes, mvr_ctx.hip): pass k+1's whole launch chain is enqueued while pass k runs, behind
  // a gate the host opens after its solve; the poses reach the kernels through a device table instead of kernel arguments
  int pipeline = 1;                                   // 0: every pass is enqueued after the previous solve (round-2 behaviour)
  int pipeline_multi_rank = 0;                        // 1: passes with a collective over more than one rank may be queued behind the gate too (off until a recorded two-GPU run says so)
  bool no_sync = false;                               // a gated chain is being enqueued: nothing may wait for the stream or reallocate (may_block)
  unsigned long long blocking_events = 0;             // how often something did wait / reallocate (a pass without any is in steady state)
  bool single_group = false;                          // the fused pass runs its pairs as ONE group for the whole ring run: a run that may queue passes ahead must not change the layout of its work buffers (and of the seeds in them) when it starts to
  bool skip_posed_pts = false;                        // ... and the posed copies' points in ORIGINAL order are not written (nothing in a fused pass reads them: ring_passes writes them once, when the stretch of queued passes ends)
  bool pose_from_table = false;                       // mvr_cloud_transform_batch ignores its T values: every destination reads Cloud::pose_dev
  double *h_pose_in = nullptr, *d_pose_in = nullptr;  // pinned, mapped: [2][views][16] poses the host writes before it opens the gate
  PoseRec *pose_tab = nullptr; size_t pose_tab_cap = 0;      // device: [2][views]
  // the chain being enqueued reads its poses from pose_in_cur (pinned) / pose_tab_cur (device records, n of them); pending: the records
  // are not filled yet -- the posing launch of the chain does it on the way (refresh_batch), any other reader calls ensure_pose_table first
  // the completion word of the chain being enqueued: stored by the final sums launch itself when that launch is the last thing
  // of the chain (signal_armed, set by the pass loop for hosts that end a pass with the fused sums on this stream; signal_sent
  // tells the loop that it needs no write-value operation behind the chain)
  uint32_t *done_counter = nullptr; uint32_t signal_seq = 0; bool signal_armed = false, signal_sent = false;
  int lazy_super = 1;                // 1 (default): posed copies that get grid-ordered coordinates leave their super boxes (read by the culled kernel alone) to flush_super_boxes(); 0: refreshed with every posing launch
  int setup_first = 1;               // plain passes: 1 (default) = the grid builds (side stream) and the pipe's set-up are enqueued BEFORE the pass's own chain instead of behind it: the first pass of a registration is host-bound either way, and the grids are then ready when the second pass wants them (12 x 200k: 2.8 + 2.1 ms -> 3.7 + 0.5)
  int pose_prep_launch = 0;          // test hook (tune key): 1 = the device pose records are always filled by the launch made for that, never by the posing launch on the way
  const double *pose_in_cur = nullptr; PoseRec *pose_tab_cur = nullptr; int pose_tab_n = 0; bool pose_tab_pending = false;
  uint32_t *gate = nullptr; bool gate_is_signal = false;     // host-writable word the stream waits on (hipStreamWaitValue32)
  uint32_t *h_done = nullptr, *d_done = nullptr;      // pinned, mapped: the stream writes the pass number here when a pass's chain has drained
  bool pipe_ops_warm = false;                         // the stream's wait-value / write-value operations have been used once
  uint32_t pipe_seq = 0;                              // passes sent through the pipe so far
  unsigned long long pipe_steady_sig = 0, pipe_steady_events = ~0ull;      // the registration whose last run ended in steady state, and blocking_events then
  std::vector<double> pass_ms;                        // wall time of every pass of the last ring run (end of the previous solve -> end of this one)
  unsigned long long piped_passes = 0;                // passes of this context whose chain was enqueued ahead of their poses (diagnostics)
  // lean posing (refresh_batch, mvr_index.hip): a queued pass whose searches will all walk the grid writes only the grid-ordered
  // coordinates and the pose record of its posed copies -- the Hilbert-ordered copy is read as QUERIES only, and every kernel of
  // such a pass poses its query as it loads it (Cloud::sorted_stale)
  int lean_pose = 1;                                  // tune key: 0 = every posing launch writes the Hilbert-ordered copy and its boxes
  bool lean_route = false;                            // the last fused pass of this context ran without a kernel that reads a posed Hilbert copy or its boxes (seeded grid walk, tail and sets on the grid, wide reverse queries): the next one, same pairs, will too
  unsigned long long lean_passes = 0;                 // passes of this context that were posed lean (stat key)
  // multi-GPU (mvr_world.cpp): an RCCL communicator (ncclComm_t; null = this context is a world of its own)
  void *comm = nullptr; bool comm_owned = false; int comm_rank = 0, comm_world = 1;
  void **comm_lender = nullptr;                       // a world's communicator is lent: where the world keeps it (cleared when it is aborted here)
  bool stream_stuck = false;                          // ncclCommAbort did not return: the stream may never drain (waits on it are bounded from then on)
  bool comm_broken = false;                           // the communicator was aborted (a peer failed or never arrived): the multi-GPU entry points refuse until a new one is set
  // PROJECTION of a rank's share on one GPU (mvr_ctx_project; tools/rank_share_bench.py): mvr_ring_run_sharded then plans as
  // rank project_rank of project_world whatever the communicator says (a world of one: the collective is really issued, its
  // peers are not there), and the rows the absent peers would have contributed are added to the table behind the all-reduce
  int project_world = 0, project_rank = 0;
  double *proj_rows = nullptr; size_t proj_rows_cap = 0, proj_rows_n = 0;
  int wait_timeout_ms = 60000;                        // how long a rank waits for a pass that contains a collective before it declares its peers lost
  // failure injection (tests; mvr_ctx_tune): the dist_pass-th sharded pass / iteration since the knob was set
  long long dist_pass = 0, inject_fail_at = -1, inject_stall_at = -1;
  uint32_t *h_stall = nullptr, *d_stall = nullptr;    // pinned word an injected stall waits on (released by comm_abort)
  long long *seq_keys = nullptr; size_t seq_keys_cap = 0;    // [Ns] signed keys with global target indices (sequential mode, target sharded)
  double *seq_row = nullptr;                                 // device: 40 doubles = one row of sums + the failure count of the iteration
  double *dist_table = nullptr; size_t dist_table_cap = 0;   // [edges][32]: this rank's rows, all-reduced in place
  // instrumentation
  bool prof = false;
  unsigned prof_mask = ~0u;                           // families that are timed (bit f = family f)
  bool prof_totals = false;                           // level 2: culled evaluations accumulate in region A, read once at drain
  std::vector<hipEvent_t> event_pool;                 // timing events are recycled, not re-created per launch
  std::vector<ProfRec> recs;
  uint64_t *h_counts = nullptr;                       // pinned: device counters copied per profiled launch
  uint64_t *h_evals = nullptr;                        // pinned [kEvalRegion]: the culled / grid kernels' running totals, copied with every iteration's moments (mvr_icp_align's `evals` statistic without a wait of its own)
  size_t h_counts_used = 0;
  uint64_t prof_launches[MVR_K_COUNT] = {0};
  double prof_ms[MVR_K_COUNT] = {0};
  double prof_work[MVR_K_COUNT] = {0};
};

constexpr int kScratchCur = MVR_MAX_SLOTS;       // ICP's input_transformed
constexpr int kScratchTmp = MVR_MAX_SLOTS + 1;   // fitness temporary

int set_error(Ctx *c, int status, const char *what, hipError_t e = hipSuccess);
// host-side stopwatch for the set-up phases (MVR_TRACE_HOST=1): prints the milliseconds since the previous mark to stderr
void host_mark(const char *what);

// an entry point of the C-ABI, and its context
#define API __attribute__((visibility("default")))
#define CTX(p) reinterpret_cast<Ctx *>(p)
bool slot_ok(int s);                          // (mvr_ctx.hip) a caller's slot number

#define MVR_HIP_TRY(ctx, expr)                                               \
  do {                                                                       \
    hipError_t _e = (expr);                                                  \
    if (_e != hipSuccess) return ::mvr::set_error((ctx), MVR_E_HIP, #expr, _e); \
  } while (0)

constexpr size_t kProfCounts = 1 << 20;   // pinned u64 slots (a culled launch takes kEvalRegion of them)

struct ProfScope {
  Ctx *c; int fam; hipEvent_t a = nullptr, b = nullptr; double work;
  const void *d_count = nullptr; int d_bytes = 0; int n_shards = 0; double per_count = 0.0;
  ProfScope(Ctx *ctx, int family, double w);
  // work is (*dev_count) * per_cnt, read back asynchronously after the launch;
  // dev_count points to a device uint32 (bytes = 4), a uint64 (bytes = 8), or,
  // with shards > 0, to `shards` u64 counters kEvalStride apart that are summed
  ProfScope(Ctx *ctx, int family, const void *dev_count, int bytes, double per_cnt, double upper_bound, int shards = 0);
  ProfScope(const ProfScope &) = delete;
  ProfScope &operator=(const ProfScope &) = delete;
  ~ProfScope();
};

// A pass enqueued behind a host-released gate must not wait for its own stream (the host would wait for itself) nor free
// what queued kernels use: every place that synchronises or reallocates asks here first.  The runner treats the error as
// "this pass is not in steady state yet" and enqueues it the ordinary way.
inline int may_block(Ctx *c, const char *what)
{
  Ctx *top = c->parent ? c->parent : c;
  ++top->blocking_events;
  if (top->no_sync) return set_error(c, MVR_E_HIP, what);
  return MVR_OK;
}
#define MVR_MAY_BLOCK(ctx, what) do { if (int rc_ = ::mvr::may_block((ctx), "not in steady state: " what)) return rc_; } while (0)

template <class T>
int ensure(Ctx *c, T *&p, size_t &cap, size_t want)
{
  if (cap >= want) return MVR_OK;
  MVR_MAY_BLOCK(c, "a work buffer has to grow");
  if (p) { (void)hipStreamSynchronize(c->stream); (void)hipFree(p); p = nullptr; cap = 0; }
  size_t ncap = want + want / 4 + 64;
  MVR_HIP_TRY(c, hipMalloc(&p, ncap * sizeof(T)));
  cap = ncap;
  return MVR_OK;
}

// rule A2's draws (mvr_hip.h): mvr_align_prerejective (mvr_feature.hip) and ransac_draw3 (mvr_ransac.h, rules P2 / C2)
__host__ __device__ inline uint64_t prerej_mix(uint64_t z)
{
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__host__ __device__ inline uint32_t prerej_draw(uint64_t seed, uint64_t i, uint64_t j, uint64_t m)
{
  return (uint32_t)(((prerej_mix(seed + 0x9E3779B97F4A7C15ull * (16ull * i + j + 1ull)) >> 32) * m) >> 32);
}

inline unsigned blocks_for(size_t n, int threads) { return (unsigned)((n + (size_t)threads - 1) / (size_t)threads); }
__device__ __forceinline__ bool finite3(const float4 v) { return isfinite(v.x) && isfinite(v.y) && isfinite(v.z); }

// one block's share of a cloud's bounding box: row[6] = {lo xyz, hi xyz} over the points this block of 256 threads strides over
// (the block of the bounding-box launches of the batched builds, blockIdx.x of gridDim.x per cloud: mvr_grid.hip, mvr_index.hip)
__device__ __forceinline__ void bbox_block_partial(const float4 *__restrict__ p, size_t cnt, float *__restrict__ row)
{
  float lo[3] = {3.0e38f, 3.0e38f, 3.0e38f}, hi[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < cnt; i += (size_t)gridDim.x * blockDim.x) {
    const float4 v = p[i];
    lo[0] = fminf(lo[0], v.x); lo[1] = fminf(lo[1], v.y); lo[2] = fminf(lo[2], v.z);
    hi[0] = fmaxf(hi[0], v.x); hi[1] = fmaxf(hi[1], v.y); hi[2] = fmaxf(hi[2], v.z);
  }
  __shared__ float sh[4][6];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
    for (int k = 0; k < 3; ++k) { lo[k] = fminf(lo[k], __shfl_xor(lo[k], o, 64)); hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], o, 64)); }
  if ((threadIdx.x & 63) == 0) for (int k = 0; k < 3; ++k) { sh[threadIdx.x >> 6][k] = lo[k]; sh[threadIdx.x >> 6][3 + k] = hi[k]; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) for (int k = 0; k < 3; ++k) { sh[0][k] = fminf(sh[0][k], sh[w][k]); sh[0][3 + k] = fmaxf(sh[0][3 + k], sh[w][3 + k]); }
    for (int k = 0; k < 6; ++k) row[k] = sh[0][k];
  }
}

// several clouds per launch (kernel arguments by value)
constexpr int kBatchClouds = 16;
// (Tp[k], when set, overrides T[k]: the pose is read from device memory -- see PoseRec)
struct XformBatch { const float4 *src[kBatchClouds]; float4 *dst[kBatchClouds]; unsigned long long n[kBatchClouds]; Mat44d T[kBatchClouds]; const Mat44d *Tp[kBatchClouds]; };
// p' = T p as mvr_cloud_transform (f64 pose, f32 result): the ONE definition, shared by the transform kernels
// and by the index refresh that poses a scan's sorted copy directly (same operations, same bits)
__device__ __forceinline__ float4 pose_point_f64(const Mat44d &T, const float4 p)
{
  const double x = p.x, y = p.y, z = p.z;
  const double d = 1.0 / (((T.m[3] * x + T.m[7] * y) + T.m[11] * z) + T.m[15]);
  float4 o;
  o.x = (float)((((T.m[0] * x + T.m[4] * y) + T.m[8] * z) + T.m[12]) * d);
  o.y = (float)((((T.m[1] * x + T.m[5] * y) + T.m[9] * z) + T.m[13]) * d);
  o.z = (float)((((T.m[2] * x + T.m[6] * y) + T.m[10] * z) + T.m[14]) * d);
  o.w = 1.0f;
  return o;
}
// a pose record's matrix as sixteen wave-uniform values (scalar registers): for the kernels that pose their own queries with
// pose_point_f64 -- the record is the same for every thread of the launch's pair
__device__ __forceinline__ Mat44d load_pose_uniform(const PoseRec *r)
{
  Mat44d T;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const double v = r->T.m[j];
    T.m[j] = __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
  }
  return T;
}
// the query at position k of a cloud that was posed lean: exactly what the full posing launch stores in its sorted[k]
__device__ __forceinline__ float4 pose_query_f64(const Mat44d &T, const float4 *__restrict__ raw, const size_t k)
{
  const float4 p = raw[k];
  float4 v = pose_point_f64(T, p);
  v.w = p.w;
  return v;
}
// the device record of a pose (PoseRec) from its 16 doubles: inverse of x -> A x + t by cofactors, in double, as make_grid_pair
// does on the host; the stretch for ANY invertible matrix (the host has checked e <= 1e-3 before it released the pass: note_pose's bar)
__device__ __forceinline__ void make_pose_rec(const double *T, PoseRec *out)
{
  PoseRec r;
  for (int j = 0; j < 16; ++j) r.T.m[j] = T[j];
  const double A[3][3] = {{T[0], T[4], T[8]}, {T[1], T[5], T[9]}, {T[2], T[6], T[10]}};
  const double det = A[0][0] * (A[1][1] * A[2][2] - A[1][2] * A[2][1]) - A[0][1] * (A[1][0] * A[2][2] - A[1][2] * A[2][0]) +
                     A[0][2] * (A[1][0] * A[2][1] - A[1][1] * A[2][0]);
  const double id = 1.0 / det;
  const double I[3][3] = {{(A[1][1] * A[2][2] - A[1][2] * A[2][1]) * id, (A[0][2] * A[2][1] - A[0][1] * A[2][2]) * id, (A[0][1] * A[1][2] - A[0][2] * A[1][1]) * id},
                          {(A[1][2] * A[2][0] - A[1][0] * A[2][2]) * id, (A[0][0] * A[2][2] - A[0][2] * A[2][0]) * id, (A[0][2] * A[1][0] - A[0][0] * A[1][2]) * id},
                          {(A[1][0] * A[2][1] - A[1][1] * A[2][0]) * id, (A[0][1] * A[2][0] - A[0][0] * A[2][1]) * id, (A[0][0] * A[1][1] - A[0][1] * A[1][0]) * id}};
  for (int rr = 0; rr < 3; ++rr) {
    for (int k = 0; k < 3; ++k) r.minv[4 * rr + k] = I[rr][k];
    r.minv[4 * rr + 3] = -(I[rr][0] * T[12] + I[rr][1] * T[13] + I[rr][2] * T[14]);
  }
  double e2 = 0.0;
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) {
      const double d = T[4 * a] * T[4 * b] + T[4 * a + 1] * T[4 * b + 1] + T[4 * a + 2] * T[4 * b + 2];
      const double x = d - (a == b ? 1.0 : 0.0);
      e2 += x * x;
    }
  const double e = fmin(sqrt(e2), 0.5);
  r.stretch = __double2float_ru((1.0 / sqrt(1.0 - e)) * (1.0 + 1e-6));
  *out = r;
}
struct RefreshBatch {
  const float4 *pts[kBatchClouds]; const uint32_t *perm[kBatchClouds]; unsigned long long n[kBatchClouds];
  float4 *sorted[kBatchClouds], *tlo[kBatchClouds], *thi[kBatchClouds], *cbox[kBatchClouds], *sbox[kBatchClouds];
  // optional: the sorted copy of the cloud this one is a posed copy of (same ordering) and the pose -- the refresh
  // then reads that copy in order and poses it, instead of gathering pts[] through the permutation
  const float4 *from[kBatchClouds]; Mat44d T[kBatchClouds]; const Mat44d *Tp[kBatchClouds];      // (Tp[k], when set, overrides T[k])
  // optional, with `from`: the source's points in original order and where their posed copies go (the transform itself,
  // done by the same launch)
  const float4 *xsrc[kBatchClouds]; float4 *xdst[kBatchClouds];
  // optional, with `from`: the cloud's points in the order of its set's cell grid (canonical coordinates) and where their posed
  // copies go -- the grid search's side of a posed copy, written by the same launch (else: refresh_grid_coords_batch)
  const float4 *graw[kBatchClouds]; float4 *gout[kBatchClouds];
  // optional, with Tp: the pose's 16 doubles where the host put them (pinned memory) -- every block reads them from THERE and block 0
  // of the cloud fills the device record Tp[k] points into (PoseRec) for the launches that follow: no launch of its own for that
  const double *Tin[kBatchClouds];
  unsigned tile_begin[kBatchClouds];       // refresh tiles from this one on (a cloud that grew at its end keeps its leading tiles)
};
static_assert(sizeof(RefreshBatch) <= 4096, "RefreshBatch travels as a kernel argument");
// index of posed copies, straight from the sources' sorted copies (culled mode; called by mvr_cloud_transform_batch).
// with_pts: also write dst->pts = T * src->pts.  handled[k] (optional) = cloud k was refreshed by this call.
int refresh_posed_batch(Ctx *c, int count, Cloud *const *dst, Cloud *const *src, const double *T, bool with_pts = false,
                        char *handled = nullptr);
int launch_transform_f64_batch(Ctx *c, int count, const float4 *const *in, float4 *const *out, const size_t *n, const double *T,
                               const Mat44d *const *Tp = nullptr);
// ensure_index for many clouds, coordinates refreshed in one launch.  keep_lean: clouds that were posed lean stay as they are
// (the caller is the fused pass, which brings them up to date itself when one of its kernels reads the arrays)
int ensure_index_batch(Ctx *c, Cloud *const *clouds, int count, bool keep_lean = false);
// the lean posing launch: only the grid-ordered coordinates and the device pose record (32 B per point instead of 64)
struct LeanPoseBatch {
  const float4 *graw[kBatchClouds]; float4 *gout[kBatchClouds]; unsigned long long n[kBatchClouds];
  const double *Tin[kBatchClouds]; const Mat44d *Tp[kBatchClouds];      // as RefreshBatch: Tin (pinned, optional) is read and block 0 fills the record Tp points into; without Tin the record itself is read
};
// sorted[] / boxes of the clouds that were posed lean, by the full refresh (pose: the device record while passes are queued
// ahead, else `T`, 16 doubles per cloud, or the cloud's own host pose); with_pts: the points in original order too
int flush_lean_sorted(Ctx *c, Cloud *const *clouds, int count, const double *T = nullptr, const float4 *const *xsrc = nullptr);

// ---- kernel launchers (mvr_nn.hip / mvr_reduce.hip / mvr_index.hip) -----------
// forward / reverse brute-force NN.  Queries: points [q_begin, q_begin+q_count)
// of `q` (direct; key ordinal = point index), or, when `qlist` != null, the
// points q[qlist[k]] for k < *qcount (device counter; q_count is then the upper
// bound used to size the grid; key ordinal = k).
int launch_nn(Ctx *c, const float4 *q, size_t q_begin, size_t q_count, const uint32_t *qlist,
              const uint32_t *qcount, const float4 *t, size_t nt, bool fma, nnkey_t *keys);

// Morton order + tile AABBs of a cloud, (re)built or refreshed as needed
int ensure_index(Ctx *c, Cloud &cl);
int flush_super_boxes(Ctx *c);                         // the super boxes the posing launches left out (lazy_super), for every cloud of the context: called by the culled launchers
void new_point_set(Ctx *c, Cloud &cl);                 // after upload / append / clear
void inherit_point_set(Cloud &dst, const Cloud &src);  // after copy / transform
// dst has just grown from old_n points by the points of `src` (appended at its end): keep dst's ordering and extend it by
// src's own, shifted -- the merged target of the sequential mode then never sorts its 2M points again.  false: not
// applicable (no ordering on either side, a shared ordering, no room): the caller falls back to new_point_set.
bool extend_point_set(Ctx *c, Cloud &dst, size_t old_n, const Cloud &src);
// culled exact NN.  Queries: sorted positions [q_begin, q_begin+q_count) of the query cloud; key ordinal = ORIGINAL
// index of the query, or -- with qflags (one byte per sorted position, only flagged positions are searched) -- the
// sorted position.  cap2: distances above it are not needed (+inf = unbounded).  The batch form runs the searches
// of several scan pairs in ONE launch (blockIdx.y = pair).
constexpr int kBatchPairs = 16;
struct CullPair {
  const float4 *qs = nullptr, *ts = nullptr, *tlo = nullptr, *thi = nullptr, *cbox = nullptr, *sbox = nullptr;
  const uint8_t *qflags = nullptr;
  const uint32_t *qlist = nullptr, *qcount = nullptr;     // compacted queries (sorted positions) and their device count
  nnkey_t *keys = nullptr;
  uint32_t q_begin = 0, q_count = 0, nt = 0, n_tiles = 0;
  const uint32_t *qbound = nullptr;   // optional, by sorted position: bits of a distance (squared) within which the query is KNOWN to have a point -- the search starts from that bound instead of the cap
  uint32_t *mark = nullptr;      // optional, with key_by_pos: [nt] start bounds of the reverse searches, by the target's sorted position (all ~0 on entry).  A query that finds a match within the cap stores the bits of its d2 at its match's position -- what a separate "flag the matched targets" launch did by re-reading all the keys.  Any matching source's distance is a valid bound: relaxed stores, last one wins.
  uint32_t key_by_pos = 0;       // plain queries only: key slot = the query's sorted position (coalesced stores) instead of its original index, AND the key's low word = the match's sorted position instead of its original index
  uint32_t seed_from_keys = 0;   // with key_by_pos: keys[] still holds the previous result of the same queries against the same target point set; every search starts from the distance of its previous match
  const uint32_t *setlist = nullptr, *setcount = nullptr;     // with qflags: the query sets that HOLD a flagged query (written by the launch that set the flags) -- launch_nn_cull_list_batch walks these instead of starting a block per set
};
struct CullBatch { CullPair p[kBatchPairs]; float cap2; };
CullPair make_cull_pair(const Cloud &q, size_t q_begin, size_t q_count, const uint8_t *qflags, const Cloud &t, nnkey_t *keys);
// block -> (pair, query set) of a fused launch, XCD-aware (see mvr_cull.hip: nn_cull_kernel)
struct XcdMap { uint32_t sets[kBatchPairs]; uint32_t n_pairs, slices; };
__host__ __device__ inline uint32_t slice_len(uint32_t sets, uint32_t slices, uint32_t slice)
{
  return sets > slice ? (sets - slice + slices - 1u) / slices : 0u;
}
__host__ __device__ inline bool xcd_map_block(const XcdMap &m, uint32_t block, uint32_t *pair, uint32_t *set)
{
  uint32_t r = block >> 3;
  for (uint32_t u = block & 7u; u < m.n_pairs * m.slices; u += 8u) {
    const uint32_t p = u / m.slices, sl = u % m.slices, len = slice_len(m.sets[p], m.slices, sl);
    if (r < len) { *pair = p; *set = sl + r * m.slices; return true; }
    r -= len;
  }
  return false;
}

inline void xcd_map_plan(XcdMap &map, int forced_slices, unsigned *grid_blocks)
{
  uint32_t g = 8u;
  while (map.n_pairs % g) g >>= 1;                            // gcd(pairs, 8)
  map.slices = 8u / g;
  if (forced_slices == 1 || forced_slices == 2 || forced_slices == 4 || forced_slices == 8) map.slices = (uint32_t)forced_slices;
  uint32_t per_xcd = 0;                                       // the longest of the 8 block lists
  for (uint32_t v = 0; v < 8u; ++v) {
    uint32_t tot = 0;
    for (uint32_t u = v; u < map.n_pairs * map.slices; u += 8u) tot += slice_len(map.sets[u / map.slices], map.slices, u % map.slices);
    per_xcd = per_xcd > tot ? per_xcd : tot;
  }
  *grid_blocks = 8u * per_xcd;
}
int launch_nn_cull_batch(Ctx *c, const CullPair *pairs, int n_pairs, float cap2, bool fma);
int launch_nn_cull_list_batch(Ctx *c, const CullPair *pairs, int n_pairs, float cap2, bool fma);     // only the query sets on the pairs' set lists (Q = 1)
// ---- grid search (mvr_grid.hip): exact 1-NN of seeded / bounded queries, one thread per query
struct GridPair {
  const float4 *qs = nullptr;                 // queries: a Hilbert-ordered posed cloud (w = original index)
  const float4 *qraw = nullptr;               // a query cloud that was posed lean: its RAW Hilbert-ordered copy -- the query is pose_point_f64(qpose_dev->T, qraw[pos]), qs[] is not read
  const uint32_t *qlist = nullptr, *qcount = nullptr;     // optional: compacted query positions + their device count (key slot = list position)
  uint32_t q_begin = 0, q_count = 0;
  const float4 *gts = nullptr;                // target: posed coordinates in GRID order (w = original index)
  const float4 *ts = nullptr;                 // target in Hilbert order (only to price the seed: the previous match's position)
  const uint32_t *start = nullptr, *g2h = nullptr, *h2g = nullptr, *tinv = nullptr;      // (tinv: original index -> Hilbert position in the searched cloud)
  const uint32_t *dir = nullptr, *recs = nullptr;      // the compact form of the cell starts (CellGrid): used when dir is set
  int dtdim[3] = {1, 1, 1};
  const uint8_t *dt = nullptr;
  float lo[3] = {0, 0, 0}, inv_h = 1.f, h = 1.f;
  int dim[3] = {1, 1, 1};
  uint8_t *heavy = nullptr;                   // optional, by query position (by LIST position with qlist): a query whose ball spans more than `light_rows` rows of cells is NOT answered here but flagged (1, else 0) for the culled kernel, which is built for wide searches
  double minv[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};     // posed frame -> canonical frame of the target: r = minv (3 x 4, row-major) * (p, 1)
  uint32_t nt = 0;
  nnkey_t *keys = nullptr;
  const uint32_t *qbound = nullptr;           // optional start bounds by query position (bits of a d2; ~0 = none)
  uint32_t *mark = nullptr;                   // optional: start bounds of the reverse searches, by the match's Hilbert position
  uint32_t key_by_pos = 0, seed_from_keys = 0;
  const PoseRec *pose_dev = nullptr;     // optional: minv / stretch are read from here (device-visible) instead of the two by-value members
  const PoseRec *qpose_dev = nullptr;    // ... and the QUERY cloud's record (with qraw: the pose its queries are posed with)
  float stretch = 1.f;                   // distances in the searched cloud's canonical frame are at most this times the posed ones (Cloud::pose_stretch, rounded up)
  int dt_max = 12;                       // what dt == 255 stands for (the grid's dt_steps)
  // a BOUNDED query whose ball is wide (scattered among the others: a match that moved far, a long correspondence) is
  // neither walked by its own thread (the wave would wait for it) nor flagged for the culled kernel (one such query
  // per 64 would wake every block): its ordinal is appended here and a second launch gives each of them a whole wave
  uint32_t *wide_list = nullptr, *wide_count = nullptr;
  uint32_t *cull_sets = nullptr, *cull_count = nullptr;      // with heavy, one lane per query: the 64-query sets that hold a flagged query (what launch_nn_cull_list_batch walks)
};
constexpr int kGridBatchPairs = 12;
constexpr int kWideCounters = 64;          // pairs of one fused pass that can have wide lists (more: the pass takes the culled kernel)
constexpr int kGridDtMax = 12;        // most dilation steps of the distance map (a grid is built with as many as the first search radius it serves needs)
constexpr int kGridLightRows = 24;    // default number of rows of cells (x-runs) a thread walks by itself (with the probe at its own threshold of 12 rows: 24 takes 0.19 ms off the first four passes of a window that restarts from the prior, settled passes equal; 32 and 48 within 2 % of it; before the probe had a threshold of its own, on the 12 x 200k ring: 9..16 equal, 4 and 27 slower)
struct GridBatch { GridPair p[kGridBatchPairs]; float cap2; int light_rows; int cluster = 65; int probe = 0; int probe_rows = 1 << 30; };
int launch_nn_grid_batch(Ctx *c, const GridPair *pairs, int n_pairs, float cap2, bool fma);
int launch_nn_grid_wide_batch(Ctx *c, const GridPair *pairs, int n_pairs, float cap2, bool fma);
int launch_nn_grid_tail_batch(Ctx *c, const GridPair *pairs, int n_pairs, float cap2, bool fma);     // the two launches below in one
int launch_nn_grid_sets_batch(Ctx *c, const GridPair *pairs, int n_pairs, float cap2, bool fma);     // the 64-query sets the first launch listed (flagged queries only): a block per set over the grid     // the queries the first launch put on the wide lists
// the set's grid (built from `canon`, a cloud holding the set's canonical coordinates) and the posed copy's grid-ordered
// coordinates; false = not available (the caller uses the culled kernel)
int cloud_bbox(Ctx *c, const float4 *pts, size_t n, float out[6], bool finite_only = false);      // {lo xyz, hi xyz} on the host (synchronises the stream); finite_only: over the points without a NaN or an infinity (none: lo > hi)
bool ensure_grid(Ctx *c, Cloud &canon, double reach);
int ensure_model_grid(Ctx *c, Cloud &t, bool *ok, bool *no_finite = nullptr);      // the grid of a cloud over its own coordinates (Cloud::mgrid); *no_finite: refused because no point of the cloud is finite
int ensure_grids(Ctx *c, Cloud *const *canon, int count, double reach, hipStream_t on, hipEvent_t after);      // the same for many sets at once, enqueued on `on` (no wait afterwards)      // reach: the search radius the distance map should be able to rule out (mm)
int refresh_grid_coords_batch(Ctx *c, Cloud *const *posed, int count);
int ensure_pose_table(Ctx *c);      // (mvr_ctx.hip) fills the device pose records of the chain being enqueued if nobody has yet
// can the posed cloud's grid-ordered coordinates be written now (grid there and ready, buffer, position maps)?  Queues what that needs
// on the context's stream; the caller then writes gsorted[] and sets gcoords_valid.
int grid_coords_prepare(Ctx *c, Cloud *cl, bool *ok);
int flush_g2h(Ctx *c);      // launches what grid_coords_prepare queued (grid position <-> Hilbert position maps), all grids in one launch      // (*ok = false: no grid to write for; the return value is a status)
// the pipelined pass loop shared by mvr_ring_run and mvr_ring_run_sharded (mvr_ctx.hip).  enqueue(): one pass's GPU work on
// c->stream, ending with the edge table on its way to c->h_table; solve(): the host step on c->h_table, poses in / out.
struct PassLoop {
  int n_views = 0; const int *posed_slots = nullptr, *raw_slots = nullptr; double *poses = nullptr;     // poses: [views][16], in / out
  int (*enqueue)(void *self) = nullptr; int (*solve)(void *self) = nullptr; void *self = nullptr;
  bool ends_with_sums = false;      // enqueue()'s last operation on the stream is the fused sums launch writing the host's table (it may carry the completion word)
  double reach = 0.0;              // the search radius of the passes (mm): with it the loop builds the scans' grids while the first pass searches
  unsigned long long sig = 0;      // identifies the registration (slots, point sets, edges, parameters): a run that ended in steady state lets the next run of the SAME registration start pipelined
};
unsigned long long pass_loop_sig(Ctx *c, int n_views, const int *posed_slots, const int *raw_slots, int ne, const int *edge_src, const int *edge_tgt,
                                 double max_dist, int reciprocal, int fma, int extra);
int ring_passes(Ctx *c, int n_steps, const PassLoop &loop, double timing_ms[3]);
// ---- collectives of a context (mvr_world.cpp); every one of them is a no-op returning MVR_OK without a communicator
enum { kReduceMinI64 = 0, kReduceSumF64 = 1 };
int comm_allreduce(Ctx *c, void *dev_buf, size_t count, int kind);      // in place, on the context's stream
int comm_poll(Ctx *c, bool abort_now = true); // RCCL's asynchronous error state; an error aborts the communicator (abort_now) -> MVR_E_RCCL
bool drain_bounded(Ctx *c, int ms);           // hipStreamSynchronize -- bounded by ms once an abort has failed to free the stream (Ctx::stream_stuck)
int comm_abort(Ctx *c, const char *why);      // ncclCommAbort + release of anything that could hold the stream; returns MVR_E_RCCL
int stream_wait(Ctx *c);                      // hipStreamSynchronize; with a communicator: bounded by wait_timeout_ms and watching comm_poll, a timeout aborts
GridPair make_grid_pair(const Cloud &q, size_t q_begin, size_t q_count, const Cloud &t, nnkey_t *keys);
int launch_nn_cull(Ctx *c, const Cloud &q, size_t q_begin, size_t q_count, const uint8_t *qflags, const Cloud &t, float cap2,
                   bool fma, nnkey_t *keys);
// one scan pair of a batched global pass (mvr_pair_moments2_batch, culled mode): everything the glue and the
// reduction kernels need, by value (blockIdx.y = pair)
struct GluePair {
  const float4 *src = nullptr, *tgt = nullptr;            // original-order points
  const float4 *qs = nullptr, *ts = nullptr;              // the same points in index (Hilbert) order, w = original index
  const float4 *qraw = nullptr, *traw = nullptr;          // by_pos, a cloud that was posed lean: its raw Hilbert-ordered copy and its device pose record instead (see GridPair::qraw)
  const PoseRec *qrec = nullptr, *trec = nullptr;
  const nnkey_t *keys = nullptr, *rkeys = nullptr;        // forward keys [ns] (by original index, or by sorted position: by_pos), reverse keys [nt] (by sorted position)
  const uint32_t *qperm = nullptr, *tinv = nullptr;
  uint8_t *flags = nullptr;                               // [nt], sorted target space
  uint32_t *bound = nullptr;                              // instead of flags: [nt] bits of a matching d2 per target (~0 = not matched)
  uint32_t *list = nullptr, *slot = nullptr;              // [<= nt] flagged sorted positions in order; [nt] position -> list index
  uint32_t *chunks = nullptr, *qcount = nullptr;          // [ceil(nt / 256)] flagged per chunk -> exclusive offsets; number flagged
  unsigned long long nt = 0;
  double *partials = nullptr, *out = nullptr;             // [blocks][29] scratch, 32 doubles result
  unsigned long long q_begin = 0, q_count = 0;
  int blocks = 0, by_pos = 0;
  uint32_t *zero_a = nullptr, *zero_b = nullptr, *zero_c = nullptr;          // optional: two device words the moments launch resets to 0 (the grid search's wide-list counters of this pair)
};
struct GlueBatch {
  GluePair p[kBatchPairs]; double max2; double origin[3]; int reciprocal;
  // optional: the LAST block of the final sums launch to finish stores done_seq into done_word (pinned host memory): the
  // host of a pipelined pass loop learns from the kernel itself that the pass's table is complete, instead of from a
  // stream write-value operation queued behind it (a packet of its own: 4 us + a 9 us gap on the critical path)
  uint32_t *done_word = nullptr, *done_counter = nullptr; uint32_t done_seq = 0;
};
int launch_flag_matched_batch(Ctx *c, const GlueBatch &b, int n_pairs);
int launch_compact_flags_batch(Ctx *c, const GlueBatch &b, int n_pairs);      // flags -> ordered list / slot / count, 3 launches for all pairs
int launch_accept_moments2_batch(Ctx *c, const GlueBatch &b, int n_pairs);
int launch_add_f64(Ctx *c, double *dst, const double *src, size_t n);      // dst[i] += src[i] (one small launch)
int reduce_blocks_for(const Ctx *c, size_t n);

// the same flags compacted (ordered) into list[] with count and the inverse slot[] (sorted position -> list position)
int launch_mark_sorted(Ctx *c, const nnkey_t *keys, const uint32_t *qperm, size_t q_begin, size_t q_count, double max2,
                       const uint32_t *tinv, size_t nt, uint8_t *flags, uint32_t *list, uint32_t *count, uint32_t *slot);
// bound[sorted target position] = bits of the forward d2 of a source that matched it (~0: none): where the reverse search of a matched target starts
// seeds of an align's forward searches (mvr_cull.hip): bound[q] = bits of the distance from query q (sorted position) to target point
// seed[q] (sorted position; >= nt: none -> ~0), with the searches' own formula; and the seeds an align leaves behind: the sorted
// position of every query's match (keys by ORIGINAL index, low word = the match's original index)
int launch_seed_to_bound(Ctx *c, const float4 *qs, size_t nq, const float4 *ts, size_t nt, const uint32_t *seed, bool fma, uint32_t *bound);
int launch_keys_to_seed(Ctx *c, const float4 *qs, size_t nq, const nnkey_t *keys, const uint32_t *tinv, uint32_t *seed);
int launch_seed_bounds(Ctx *c, const nnkey_t *keys, const uint32_t *qperm, size_t q_begin, size_t q_count, double max2,
                       const uint32_t *tinv, size_t nt, uint32_t *bound, uint32_t *seed_out = nullptr, uint32_t *zero_word = nullptr);
// culled-mode reciprocal glue: flag the matched targets (one byte per sorted target position)
int launch_flag_matched(Ctx *c, const nnkey_t *keys, const uint32_t *qperm, size_t q_begin, size_t q_count, double max2,
                        const uint32_t *tinv, size_t nt, uint8_t *flags);

// All scratch arrays of a denoise / voxel-grid call are carved out of ONE grow-only buffer kept by the context, Ctx::dn_arena
// (twelve hipMalloc + hipFree per call cost more than the kernels: 5.3 ms per 204k-point scan, 1.5 ms of it on the GPU):
// plan() the arrays to size the buffer, then take() them in the same order (or fewer / smaller ones).
struct Carver {
  char *base = nullptr;
  size_t off = 0;
  template <class T> void plan(size_t count) { off = ((off + 255) & ~(size_t)255) + std::max<size_t>(count, 1) * sizeof(T); }
  template <class T> T *take(size_t count)
  {
    off = (off + 255) & ~(size_t)255;
    T *p = reinterpret_cast<T *>(base + off);
    off += std::max<size_t>(count, 1) * sizeof(T);
    return p;
  }
};
// a device allocation (through the pool) that lives as long as a call (mvr_feature.hip, mvr_pfh.hip, mvr_radius.hip)
struct DevBuf {
  void *p = nullptr;
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  ~DevBuf() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 1); }
  template <class T> T *as() const { return reinterpret_cast<T *>(p); }
};

// grows a cloud's point buffer to `cap` points (keep: its current points are copied over)
int cloud_reserve(Ctx *c, Cloud &cl, size_t cap, bool keep);

// PointCloud::denoise (mvr_denoise.hip): the cloud is replaced by its kept points, in the reference's output order
int denoise_cloud(Ctx *c, Cloud &cl, int segment_threshold, double triangle_length, size_t *n_kept, size_t *n_components,
                  uint32_t *host_index);
// ---- the tail of a filter that keeps a subset (mvr_denoise.hip), in the order its callers run it
// mark_index_kernel: flags[d_index[k]] = value for k < count, a caller's index list (on the device) into a flag per point
int launch_mark(Ctx *c, const uint32_t *d_index, size_t count, uint8_t value, uint8_t *flags);
// flags -> list[] = the indices of the set flags, ascending, and *count (a device word) = how many: hipCUB's
// DeviceSelect::Flagged.  tmp null: only tmp_bytes = the temporary storage a call over n flags needs
int select_flagged(Ctx *c, void *tmp, size_t &tmp_bytes, const uint8_t *flags, size_t n, unsigned long long *list, uint32_t *count);
// gather_kernel: out[k] = in[low word of okey[k]] for k < kept, and index_out[k] (optional) = that index -- points and normals alike
int launch_gather(Ctx *c, const float4 *in, const unsigned long long *okey, size_t kept, float4 *out, uint32_t *index_out);
// dst's points become pts[list[k]], k < kept, and (nrm set) its normals nrm[list[k]]; index_out as launch_gather.  pts / nrm
// may be dst's own arrays (a filter in place: gathered through `stage`, kept elements, and copied back) or any others (dst's
// arrays are grown to `kept`).  All of it queued on the context's stream.
int gather_kept(Ctx *c, Cloud &dst, const float4 *pts, const float4 *nrm, const unsigned long long *list, size_t kept, float4 *stage,
                uint32_t *index_out);
// the output replaces dst's points: a new point set of n points (as after an upload)
void finish_dst(Ctx *c, Cloud &dst, size_t n, bool normals);
// pcl::VoxelGrid::filter (mvr_voxel.hip; rules at mvr_cloud_voxel_grid in mvr_hip.h): dst (which may be src) gets the voxel
// centroids as a new point set
int voxel_grid_cloud(Ctx *c, Cloud &dst, Cloud &src, const float leaf[3], unsigned min_points, size_t *n_out, uint32_t *voxel_of,
                     int *passthrough);
// the first four steps of voxel_grid_cloud for a cubic leaf (mvr_voxel.hip), for the callers that need the voxels' members and
// not their centroids (mvr_ndt.hip): the lattice, then the finite points sorted by 64-bit voxel index (stable: a voxel's members
// in ascending point order), the segment heads and their inclusive scan, all carved from `s` (voxel_sorted_plan sizes them).
struct VoxLattice {
  float inv[3], minbf[3];
  unsigned long long div[3], sentinel;      // div0 div1 div2 <= sentinel: one past the largest index
  size_t nf;                                // finite points (0: no voxel; the rest is not set)
  bool pass;                                // rule 3: the lattice is too large
  int bits;
};
struct VoxSorted { const unsigned long long *key; const uint32_t *idx, *head, *vid; };
void voxel_sorted_plan(Ctx *c, size_t n, Carver &plan);
int voxel_sorted_index(Ctx *c, const Cloud &src, float leaf, Carver &s, VoxLattice *lat, VoxSorted *out);
int launch_fill_u64(Ctx *c, nnkey_t *p, size_t n, nnkey_t v);
// keys with LOCAL target indices <-> signed 64-bit keys with GLOBAL target indices (what a MIN all-reduce over
// ranks combines; "no neighbour" = INT64_MAX).  import keeps only the matches this shard owns.
int launch_export_keys(Ctx *c, const nnkey_t *keys, size_t n, const SegTable &st, long long *out);
int launch_import_keys(Ctx *c, const long long *in, size_t n, const SegTable &st, nnkey_t *keys);
int launch_mark(Ctx *c, const nnkey_t *keys, size_t q_begin, size_t q_count, double max2,
                uint32_t *slot, uint32_t *list, uint32_t *count);
// The per-query kernels walk positions [q_begin, q_begin+q_count) and take the
// query index i = qperm ? qperm[pos] : pos.  slot is indexed by tinv ? tinv[j] : j.
// pass 1: match[] + {n, sum p, sum q, sum d2}; then means into moments[0..7]
int launch_pass1(Ctx *c, const float4 *src, const float4 *tgt, const nnkey_t *keys,
                 const nnkey_t *rkeys, const uint32_t *slot, const uint32_t *count, const uint32_t *qperm,
                 const uint32_t *tinv, size_t q_begin, size_t q_count, double max2, bool reciprocal,
                 int32_t *match, double *moments);
// pass 2: sigma = (1/n) sum (q-mean_q)(p-mean_p)^T into moments[8..16]
int launch_pass2(Ctx *c, const float4 *src, const float4 *tgt, const int32_t *match, const uint32_t *qperm,
                 size_t q_begin, size_t q_count, double *moments, const unsigned long long *eval_totals = nullptr,
                 double *host_out = nullptr, uint32_t host_seq = 0);      // host_out: mapped pinned memory that receives moments[0..18] and, at double 64, the word host_seq
// raw second moments about `origin` into out[0..31] (device pointer)
int launch_accept_moments2(Ctx *c, const float4 *src, const float4 *tgt, const nnkey_t *keys, const nnkey_t *rkeys,
                           const uint32_t *slot, const uint32_t *qperm, const uint32_t *tinv, size_t q_begin, size_t q_count,
                           double max2, bool reciprocal, const double origin[3], double *out);
int launch_moments2(Ctx *c, const float4 *src, const float4 *tgt, const int32_t *match, const nnkey_t *keys, const uint32_t *qperm,
                    size_t q_begin, size_t q_count, const double origin[3], double *out);
// K10 (extension): point-to-plane normal equations over the accepted pairs:
// out[0..20] = upper triangle of sum a a^T (a = [p x n, n]), out[21..26] = sum a*d,
// out[27] = count, out[28] = sum d^2  (d = n . (q - p)); device pointer
int launch_p2plane(Ctx *c, const float4 *src, const float4 *tgt, const float4 *tnrm, const int32_t *match,
                   const uint32_t *qperm, size_t q_begin, size_t q_count, double *out);
// ---- correspondence rejectors (mvr_reject.hip; rules R1-R10 at mvr_correspondences_rejected in mvr_hip.h)
// Layout of Ctx::rej_row: doubles [0, kRejRowDoubles) = the iteration's sums; then uint32 words: [0] the number found, then
// kRejStageWords per stage {out, threshold bits, prefix, rank, none, pad...}; the copy to the host ends there.  Behind it the
// radix histogram and the per-block tie counts.
constexpr int kRejRowDoubles = 64, kRejStageWords = 8, kRejHeadWords = 8;
constexpr int kRejCopyWords = kRejHeadWords + MVR_MAX_REJECTORS * kRejStageWords;
constexpr int kRejHistBins = 2048, kRejTieBlocks = 1024;
constexpr size_t kRejCopyBytes = (size_t)kRejRowDoubles * sizeof(double) + (size_t)kRejCopyWords * sizeof(uint32_t);
constexpr size_t kRejRowBytes = kRejCopyBytes + (size_t)(kRejHistBins + kRejTieBlocks) * sizeof(uint32_t);
int ensure_reject_state(Ctx *c, size_t nt, bool one_to_one);
// the chain over keys[] / match[] (ns entries, by source index) in place: a rejected entry gets match = -1.  found: a device
// double holding the number live at entry (pass 1's moments[0]), or null: found_host.  Nothing comes to the host.
// spts / tpts / fma / trace: what a SAMPLE_CONSENSUS stage needs (rules C1-C12) -- that stage alone synchronises the stream.
int launch_reject_chain(Ctx *c, const mvr_rejector *chain, int n_chain, const nnkey_t *keys, int32_t *match, size_t ns, size_t nt,
                        const float4 *snrm, const float4 *tnrm, const double *found, uint32_t found_host, const float4 *spts = nullptr,
                        const float4 *tpts = nullptr, bool fma = false, mvr_rej_sac_trace *sac_trace = nullptr, size_t sac_trace_cap = 0);
// ---- the sample-consensus rejector (mvr_reject_sac.hip; rules C1-C12 at mvr_reject_sample_consensus in mvr_hip.h)
// one stage over match[] (ns entries) in place; `stage` = the stage's device words (word 0 receives the number kept).  Leaves
// its result in Ctx::last_sac.
int reject_sac_stage(Ctx *c, const mvr_rejector &r, bool fma, const float4 *src, const float4 *tgt, int32_t *match, size_t ns, uint32_t *stage,
                     mvr_rej_sac_trace *trace, size_t trace_cap);
void reject_sac_identity(mvr_rej_sac_result *R);      // found = 0, T = identity
// ---- Generalized ICP (mvr_gicp.hip; rules G1-G10 at mvr_icp_align_gicp in mvr_hip.h)
// Layout of Ctx::gicp_state, in doubles: X (R row-major, t), the candidate Xc, the 29 sums at X, lambda, the objective per
// correspondence at identity and at X, the norms of the step that made the candidate; then four uint32 words.
constexpr int kGicpX = 0, kGicpXc = 12, kGicpSums = 24, kGicpLambda = 53, kGicpF0 = 54, kGicpF1 = 55, kGicpStepRot = 56,
              kGicpStepTrans = 57, kGicpWordsAt = 58, kGicpStateDoubles = 64;
constexpr int kGicpEvals = 0, kGicpAccepted = 1, kGicpDone = 2, kGicpStatus = 3;
constexpr size_t kGicpStateBytes = (size_t)kGicpStateDoubles * sizeof(double);
int ensure_gicp_state(Ctx *c);
// the state block at X (column-major 4x4, or null: identity), lambda = 1e-3, counters and `done` cleared
int launch_gicp_init(Ctx *c, const double X[16]);
// `pairs` evaluation + step launches over match[] (q_count entries from q_begin, through qperm if given); sums_only: one
// evaluation whose 29 sums are left at kGicpSums (p may be null)
int launch_gicp_pairs(Ctx *c, const float4 *src, const float4 *snrm, const float4 *tgt, const float4 *tnrm, const int32_t *match,
                      const uint32_t *qperm, size_t q_begin, size_t q_count, const mvr_gicp_params *p, double eps, bool sums_only,
                      int pairs);
int read_gicp_state(Ctx *c);                       // state block -> Ctx::gicp_host, synchronised
// the whole inner optimisation (G7) from X = I; `ride` (optional) queues the caller's own copies before the first round trip
int gicp_optimise(Ctx *c, const float4 *src, const float4 *snrm, const float4 *tgt, const float4 *tnrm, const int32_t *match,
                  const uint32_t *qperm, size_t q_begin, size_t q_count, const mvr_gicp_params *p, int (*ride)(Ctx *));
// ---- Normal Distributions Transform (mvr_ndt.hip; rules N1-N12 at mvr_ndt_align in mvr_hip.h)
// the kept cells of a target, in the context's arena (valid until the next call that carves it), and how to find one
struct NdtCells {
  const unsigned long long *key = nullptr; const uint32_t *count = nullptr; const double *mean = nullptr, *icov = nullptr;
  uint32_t n = 0;
  const uint32_t *table = nullptr;          // dense route: voxel -> cell or kNone; null: search `key`
  VoxLattice lat;
};
// what an evaluation needs besides the cells: G (R row-major, t), o, t, R, the three first and six second derivatives of R
// (rx, ry, rz; then xx xy xz yy yz zz), the constants of N2 and the squared radius
struct NdtPose { double G[12], o[3], t[3], R[9], D[3][9], DD[6][9], d1, d2, r2; };
int ndt_args(const mvr_ndt_params *p, const double *guess, double d123[3], const char **why);      // N11's parameter checks (host_math.cpp; why: what was refused)
void ndt_pose(const mvr_ndt_params *p, const double d123[3], const double *guess, const double x[6], NdtPose *P);
void ndt_matrix(const NdtPose &P, double X[16]);                                         // X(p) G, column-major
int ndt_build_cells(Ctx *c, const Cloud &tgt, const mvr_ndt_params *p, NdtCells *cells);
int ndt_eval(Ctx *c, const Cloud &src, const NdtCells &cells, const NdtPose &P, double out[29]);      // two launches and one read-back
int ndt_direction(const double sums[29], double delta[6]);                               // N7 (host_math.cpp)
int ndt_newton(const mvr_ndt_params *p, mvr_ndt_eval_fn eval, void *user, double p_out[6], double sums_out[29], mvr_ndt_stats *st,
               mvr_ndt_iter_trace *trace, int trace_cap);                                  // N7-N9 on a callback's sums (host_math.cpp)
// ---- the search of one pair (mvr_ctx.hip), as the aligns of mvr_align.hip drive it
// what a search leaves for pass 1.  qperm / tinv: the culled mode's orderings; slot / count: the brute-force mode's compacted
// reverse queries (the culled mode searches the flagged targets in place: reverse keys are indexed by sorted target position)
struct SearchPlan { const uint32_t *qperm = nullptr; const uint32_t *tinv = nullptr; const uint32_t *slot = nullptr; const uint32_t *count = nullptr; };
int run_search(Ctx *c, Cloud &src, Cloud &tgt, size_t qb, size_t qn, double max_dist, bool reciprocal, bool fma, double *evals, SearchPlan *plan);
int pair_common(Ctx *c, int ss, int ts, double max_dist, int reciprocal, int fma, size_t qb, size_t qn, double *evals, SearchPlan *plan);
int forward_keys_impl(Ctx *c, Cloud &s, Cloud &t, double max_dist, int fma, long long *dev_keys);
int moments2_from_keys_impl(Ctx *c, Cloud &s, Cloud &t, const long long *dev_keys, double max_dist, int reciprocal, int fma,
                            const double origin[3], double *dev_out);
float cap_from_max2(double max2);             // smallest float bound that admits every float d2 with (double)d2 <= max2
int read_moments(Ctx *c, size_t n_doubles);   // Ctx::moments -> h_moments, synchronised
int ensure_align_row(Ctx *c);                 // the mapped pinned row an align's last sums launch writes itself ...
int spin_moments(Ctx *c, uint32_t seq, size_t n_doubles);      // ... and the wait for its word `seq`; the row lands in h_moments
double now_ms();
int launch_rotate_normals_f32(Ctx *c, const float4 *in, float4 *out, size_t n, const float T[16]);
int launch_rotate_normals_f64(Ctx *c, const float4 *in, float4 *out, size_t n, const double T[16]);
int launch_fitness(Ctx *c, const nnkey_t *keys, size_t n, double max_range, double *moments);
int launch_transform_f32(Ctx *c, const float4 *in, float4 *out, size_t n, const float T[16]);
int launch_transform_f64(Ctx *c, const float4 *in, float4 *out, size_t n, const double T[16]);
int launch_unpack_xyz(Ctx *c, const float *packed, float4 *out, size_t n);
int launch_pack_xyz(Ctx *c, const float4 *in, float *packed, size_t n);
int launch_decode_keys(Ctx *c, const nnkey_t *keys, size_t n, uint32_t *idx, float *d2);

// ---- host math (host_math.cpp) ------------------------------------------------
void svd3(const double A[9], double U[9], double S[3], double V[9]);
void umeyama_from_moments(const double mean_src[3], const double mean_tgt[3],
                          const double sigma[9], float T[16], double sv[3]);
// pcl TransformationEstimationPointToPlaneLLS: x = (A^T A)^-1 A^T b, T = Rz(g) Ry(b) Rx(a) + t
int p2plane_solve(const double ata_upper[21], const double atb[6], float T[16]);
int invert6(const double A[36], double Ainv[36]);
int solve_dense(int n, double *A, double *b);

}  // namespace mvr
