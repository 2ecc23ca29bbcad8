// tl_ctx.hpp -- host-side context of the C ABI (include/tloam_hip.h), shared by the API translation units (tl_api.hip:
// lifetime, tl_api_frames.hip: HBM residency + search grids, tl_api_match.hip: the scanMatching driver, tl_api_sets.hip: its factor set outside a frame, tl_api_comm.hip: multi-GPU
// exchange, tl_api_submap.hip: device-resident submap, tl_api_feature.hip: PCA features, tl_api_seg.hip: segmentation,
// tl_api_odom.hip: the whole odometry frame, tl_api_map.hip: its global map and registered scan, tl_api_vmap.hip: its merged
// voxel map, tl_api_deskew.hip: its deskew, tl_api_place.hip: place recognition, tl_api_cmap.hip: the closed map, tl_api_carve.hip: its carve,
// tl_api_surfel.hip: its surfels, tl_api_snapshot.hip: its snapshot).
// Memory: every buffer below belongs to the struct that declares it and dies with it (the owning types come first).
#pragma once

#include <dlfcn.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <initializer_list>
#include <memory>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "tl_common.hpp"
#include "tl_seg.hpp"
#include "tl_tile_box.hpp"


namespace tlh {
using namespace tl;


// ------------------------------------------------------------------------------------------------
//  who owns memory: a device or pinned-host buffer belongs to the struct that declares it and is freed when that struct dies --
//  with the context (tloam_destroy's `delete`), with a function's locals, or where a state is assigned a fresh value to give
//  its memory back mid-life.  Nothing lists buffers to free them.  The owners are DBuf, Retired and Pinned below (move-only:
//  a moved-from owner is empty); none is ever global or static, so none outlives the runtime.
// ------------------------------------------------------------------------------------------------
//  grow-only device buffer
template <class T>
struct DBuf {
  T* p = nullptr;
  size_t cap = 0;  // elements
  DBuf() = default;
  DBuf(DBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
  DBuf& operator=(DBuf&& o) noexcept {
    if (this != &o) {
      release();
      p = std::exchange(o.p, nullptr);
      cap = std::exchange(o.cap, 0);
    }
    return *this;
  }
  ~DBuf() { release(); }
  hipError_t reserve(size_t n) {
    if (n <= cap) return hipSuccess;
    size_t want = std::max(n, cap + cap / 2);
    want = (want + 63) & ~size_t(63);
    T* q = nullptr;
    hipError_t e = hipMalloc((void**)&q, want * sizeof(T) + 256);
    if (e != hipSuccess) return e;
    static const bool trace = getenv("TLOAM_DEBUG_ALLOC") != nullptr;   // development aid: (re)allocations inside the timed path show up here
    if (trace) fprintf(stderr, "[tloam alloc] %zu -> %zu elements of %zu B\n", cap, want, sizeof(T));
    if (p) (void)hipFree(p);
    p = q;
    cap = want;
    return hipSuccess;
  }
  // ... for a table that must read zero before its first use: zeroed as a whole, on the stream, whenever it is (re)allocated
  hipError_t reserve_zeroed(size_t n, hipStream_t s) {
    const size_t before = cap;
    const hipError_t e = reserve(n);
    return (e != hipSuccess || cap == before) ? e : hipMemsetAsync(p, 0, cap * sizeof(T), s);
  }
  void release() {   // the early free, for the places that give memory back mid-life
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

// device storage a regrowth replaced: freed once the stream has drained, the launches in flight may still read it
struct Retired {
  std::vector<void*> p;
  Retired() = default;
  Retired(Retired&& o) noexcept : p(std::move(o.p)) { o.p.clear(); }
  Retired& operator=(Retired&& o) noexcept {
    if (this != &o) {
      release();
      p = std::move(o.p);
      o.p.clear();
    }
    return *this;
  }
  ~Retired() { release(); }
  template <class T>
  void take(DBuf<T>& b) {
    if (b.p) p.push_back(b.p);
    b.p = nullptr;
    b.cap = 0;
  }
  void release() {
    for (void* q : p) (void)hipFree(q);
    p.clear();
  }
  bool empty() const { return p.empty(); }
};

// pinned host memory: `n` elements allocated with the flags given, and -- after map() -- the address the device reads them at.
// Reads as the host pointer
template <class T>
struct Pinned {
  T* h = nullptr;     // as the host reads it
  T* dev = nullptr;   // as the device addresses it (nullptr: not mapped)
  size_t n = 0;       // elements
  Pinned() = default;
  Pinned(Pinned&& o) noexcept : h(std::exchange(o.h, nullptr)), dev(std::exchange(o.dev, nullptr)), n(std::exchange(o.n, 0)) {}
  Pinned& operator=(Pinned&& o) noexcept {
    if (this != &o) {
      release();
      h = std::exchange(o.h, nullptr);
      dev = std::exchange(o.dev, nullptr);
      n = std::exchange(o.n, 0);
    }
    return *this;
  }
  ~Pinned() { release(); }
  hipError_t alloc(size_t count, unsigned flags) {   // (what it held goes first)
    release();
    const hipError_t e = hipHostMalloc((void**)&h, count * sizeof(T), flags);
    if (e != hipSuccess) h = nullptr;
    else n = count;
    return e;
  }
  hipError_t map() {
    const hipError_t e = hipHostGetDevicePointer((void**)&dev, h, 0);
    if (e != hipSuccess) dev = nullptr;
    return e;
  }
  void zero() { memset(h, 0, n * sizeof(T)); }
  void release() {
    if (h) (void)hipHostFree(h);
    h = dev = nullptr;
    n = 0;
  }
  operator T*() const { return h; }
  T* operator->() const { return h; }
};

// a pinned, device-visible segment of 8 words (mapped | coherent, zeroed) a stage's last kernel reports its result through
struct PinnedSeg : Pinned<unsigned long long> {
  hipError_t alloc() {   // (kept if there is one)
    if (h) return hipSuccess;
    hipError_t e = Pinned::alloc(8, hipHostMallocMapped | hipHostMallocCoherent);
    if (e == hipSuccess) {
      zero();
      e = map();
    }
    if (e != hipSuccess) release();
    return e;
  }
};

struct KindData {
  // source (this rank's block)
  size_t n_src_full = 0, src_lo = 0, n_src = 0;
  DBuf<double> src_aos;          // storage when the cloud came through tloam_set_source (one kind at a time)
  const double* src_ptr = nullptr;   // this rank's block of the cloud, AoS: src_aos.p, or inside the frame's src_pack (tloam_set_source_frame)
  bool src_set = false;
  // target as given by set_target
  size_t n_tgt = 0;
  DBuf<double> tgt_aos, tx, ty, tz;
  bool tgt_set = false;
  // view into the shared search-grid buffers built at sm_begin (the deep copy KDTreeFlann::SetGeometry
  // makes, :898-913)
  GridView gv{};
  bool grid_valid = false;
  // compact correspondence segment
  // ONE allocation per kind: kSegStreams arrays of `c_stride` doubles each, in the order of tl::SegStream -- K3 gets
  // the planar segment as (base, stride) in its first kernel arguments, which the command processor preloads into
  // SGPRs, so a wave can request its first chunk before any scalar load has returned
  DBuf<int> c_idx;
  DBuf<double> c_buf;
  size_t c_cap = 0, c_stride = 0;
  size_t pre_lo = 0, pre_n_full = 0;  // pre-built sets: this rank's block
};

// the clouds of one registered frame (what setInputSource / setInputTarget hand over), movable as a unit
struct FrameClouds {
  size_t n_src_full[tl::kKinds] = {}, src_lo[tl::kKinds] = {}, n_src[tl::kKinds] = {}, n_tgt[tl::kKinds] = {};
  DBuf<double> src_aos[tl::kKinds], tgt_aos[tl::kKinds], tx[tl::kKinds], ty[tl::kKinds], tz[tl::kKinds];
  DBuf<double> src_pack;                       // the four source clouds of a Frame handed over in one piece (tloam_set_source_frame)
  const double* src_ptr[tl::kKinds] = {};
  bool src_set[tl::kKinds] = {}, tgt_set[tl::kKinds] = {};
  double tgt_box[tl::kKinds][6] = {};
  bool tgt_box_valid[tl::kKinds] = {};
};

struct GridBuffers {
  DBuf<double4> gp;
  DBuf<int> cell_start, cell_of_pt, rank_of_pt;
  DBuf<unsigned long long> cell_cnt, cell_scan, scan_tmp;   // the 64-bit histogram (all-zero between builds), its scan, the scan's scratch
  DBuf<unsigned> cell_cnt32, cell_scan32, totals32;          // the frame-size path's own: 32-bit histogram (all-zero between builds), tile-local scan, tile totals
  DBuf<unsigned long long> scan1p;   // control words of the single-pass scan (large tables), zero when allocated
  DBuf<double> bbox;
};


enum CommMode { COMM_NONE = 0, COMM_CALLBACK = 1, COMM_RCCL = 2, COMM_MAILBOX = 3 };

// ---- device-resident submap (front_end.cpp:201-275): frame buffers + scratch of the crop/voxel pipeline ----
struct RingFrame {
  DBuf<double> aos;   // the frame's cloud, sensor frame, as handed over
  size_t n = 0;
  double pose[16];
};
struct SubmapState {
  bool inited = false;
  unsigned long long pending_seq = 0ull;  // sequence number the last kernel of the update in flight stores into the host slot
  tloam_submap_config cfg;
  std::vector<std::unique_ptr<RingFrame>> planar_ring, sphere_ring;  // oldest first (std::deque in the reference)
  DBuf<double> in_aos, wx, wy, wz, min_partial, vmin;
  DBuf<unsigned long long> keys, cnt, leader, leader_scan, counts;
  DBuf<int> slot_of_pt, urank, members, overflow;
};

// scratch of the PCA feature path (grow-only, kept across calls)
struct FeatBuffers {
  DBuf<double> aos, x, y, z, flatness, cvr, sphericity, normal;
  DBuf<double> f2, gf, out;        // candidate flatness of both lists ([0, n) planar, [n, 2n) sphere), grouped by bucket, ranked + packed
  DBuf<int> num_sum, neigh, idx2, gi, bkt, pos;
  DBuf<unsigned long long> flags, scan, scan_tmp;
  DBuf<tl::FeatRankCtl> rank_ctl;
  GridBuffers grid;
};

// device buffers of the segmentation node (tl_api_seg.hip; grow-only, kept across calls) and its frame counter
struct SegBuffers {
  DBuf<double> aos, pol_val, bounds, boxes, cv;
  DBuf<tl::SegCtl> ctl;
  DBuf<int> ring, cur, cur_reg, ng, reg_mem, reg_g, reg_v, ground, obj, vox, hkey, hval, parent, csize, croot, cl_root, cl_off,
      cl_size, seg_local, seg_orig, seg_label, ring_list, sorted, genbuf, edge_sec, sec_cnt, sec_base, edge, general;
  DBuf<unsigned char> reg_flag, picked;
  unsigned long long frames = 0;   // calls so far: the first one seeds minPolar / maxPolar with 5.0, later ones with 0.0
  unsigned long long aos_seq = 0;  // uploads into `aos` so far (segment_begin): what tloam_registered_scan checks residency by
};

// the odometry frame (tl_api_odom.hip): FrontEnd's state between frames and the device scratch of its glue
struct OdomState {
  bool ready = false;              // tloam_odometry_reset has been called
  tloam_odom_config cfg;
  double last[16], predict[16];    // FrontEnd::last_pose / predicate_pose (front_end.cpp:281-282, :329-332), column-major
  double step[16];                 // step_pose of the last accepted later frame (identity before): the deskew's motion
  long long frame = 0;             // frames accepted since the reset
  DBuf<double> vox_out;            // SoA output of the per-scan voxel job (edge x, y, z, then ground x, y, z) / tloam_voxel_down_sample
  DBuf<double> block;              // planar | edge | ground of the submap update (swapped into the planar ring), or the first
                                   // frame's four clouds
  DBuf<int> ctl;                   // k_odom_counts
  // the last accepted frame's registered scan (tloam_registered_scan): its scan's upload number (SegBuffers::aos_seq), its
  // size, its lidar_odom_pose (identity on the first frame, front_end.hpp:106)
  bool reg_valid = false;
  unsigned long long reg_seq = 0;
  size_t reg_n = 0;
  double reg_pose[16];
  bool reg_deskewed = false;       // its scan is the deskewed copy (DeskewState::aos), not the segmentation's input
};

// the global map of the odometry frame (tl_api_map.hip): the map itself (SoA, grown by doubling), the
// scratch of its per-frame voxel job, and the pinned segment its last kernel reports the frame's count through
struct MapState {
  tloam_map_config cfg = {0, 0, 1.0, 0};   // tloam_map_default_config until tloam_map_configure
  struct Points {
    DBuf<double> x, y, z;          // the map: n_points rows of cap
    size_t cap = 0;
  } pts;
  Retired retired;                 // storage a regrowth replaced: freed once the frame has drained the stream
  int64_t n_points = 0, n_frames = 0, last_first = 0, last_count = 0, overflow_frames = 0;
  DBuf<double> wx, wy, wz, min_partial, vmin;   // the transformed scan (kept: the registered scan of a mapping frame)
  DBuf<unsigned long long> keys, leader, counts;
  DBuf<int> head, first, count, bigslot, slot_of_pt, next, members, bigfill, ctl;
  DBuf<int4> bigq;
  PinnedSeg seg;                            // [0] voxels, [2] overflow, [7] check word
  unsigned long long seq = 0;               // numbers of the segments the map stage has posted
  unsigned long long pending_seq = 0;       // the map stage of the frame in flight (0: none)
  bool have_count = false;                  // its result, read at the frame's last wait, committed if the frame is accepted
  int64_t new_points = 0;
  bool overflowed = false;
  unsigned long long xf_seq = 0;            // upload number of the scan whose transform is in (wx, wy, wz) (0: none)
  size_t xf_n = 0;
  void clear() {   // the run's map goes; its configuration and storage stay
    n_points = n_frames = last_first = last_count = overflow_frames = 0;
    pending_seq = 0;
    have_count = false;
    xf_seq = 0;
  }
};

// voxel rows in id order and their table: the layout the merged voxel map and the closed map share (k_vmap_read / k_vmap_box
// read either: voxel_rows_of below)
struct VoxelRowStore {
  DBuf<unsigned long long> key;    // [cap] per id
  DBuf<long long> n, qx, qy, qz;   // [cap] per id
  DBuf<int> tab;                   // [tmask + 1] slot -> id, -1 free
  size_t cap = 0;
  unsigned long long tmask = 0;
  tl::VmapTable table() const {    // as the kernels see them
    tl::VmapTable T;
    T.pmask = tmask; T.ptab = tab.p; T.pkey = key.p;
    T.pn = n.p; T.pqx = qx.p; T.pqy = qy.p; T.pqz = qz.p;
    return T;
  }
  tl::VmapTableView view() const {   // ... and as the stages that only read them do
    const tl::VmapTable T = table();
    return tl::VmapTableView{T.pmask, T.ptab, T.pkey, T.pn, T.pqx, T.pqy, T.pqz};
  }
};

// the merged voxel map of the odometry frame (tl_api_vmap.hip): the persistent map in id order and its
// table (grown by doubling, rehashed from the keys), the frame's staging, and the pinned segment k_vmap_emit reports through
struct VmapState {
  tloam_voxel_map_config cfg = {0, 0, 1.0, {0.0, 0.0, 0.0}, 0};   // tloam_voxel_map_default_config until configured
  VoxelRowStore rows;
  bool tab_dirty = false;          // emptied since the table was last cleared: cleared at the next frame / read
  Retired retired;                 // storage a regrowth replaced: freed once the frame has drained the stream
  int64_t n_voxels = 0, n_points = 0, n_frames = 0, last_new = 0, overflow_frames = 0;
  // the frame's staging: its table, the slot of every point, the look-back words, control words; reads' scratch
  DBuf<unsigned long long> fkey, fsum, look, ctl;
  DBuf<int> flead, fid, slot_of_pt;
  unsigned long long fmask = 0;    // the staged frame's table size - 1
  DBuf<double> rd_c;
  DBuf<long long> rd_n;
  PinnedSeg seg;                            // [0] new voxels, [1] points, [2] overflow, [3] fault, [7] check
  unsigned long long seq = 0;
  unsigned long long pending_seq = 0;       // the stage of the frame in flight (0: none)
  bool have_count = false;                  // its result, read at the frame's last wait, committed if the frame is accepted
  int64_t new_voxels = 0, new_points = 0;
  bool overflowed = false;
  void clear() {   // the run's map goes; its configuration and storage stay
    n_voxels = n_points = n_frames = last_new = overflow_frames = 0;
    pending_seq = 0;
    have_count = false;
    if (rows.tab.p) tab_dirty = true;   // (cleared on the stream at the next frame: the ids it holds are gone)
  }
};

// the odometry frame's deskew (tl_api_deskew.hip): its configuration, the frame's corrected copy of the scan
// and its times, two max-shift words (the frame in flight writes the one the last accepted deskewed frame did not), the flag of a
// refused time; tloam_deskew_scan's own buffers
struct DeskewState {
  tloam_deskew_config cfg = {0, 0, 1, 0, 0.0, 0.0};   // tloam_deskew_default_config until tloam_deskew_configure
  DBuf<double> aos, t;
  DBuf<unsigned long long> ctl;    // [0], [1] max |p' - p| bits, [2] bad-time flag
  DBuf<double> s_in, s_out, s_t;
  DBuf<unsigned long long> s_ctl;
  bool active = false;             // the frame in flight reads its scan from `aos`
  bool timed = false;              // the frame in flight came with times
  int slot = 0;                    // the max-shift word the frame in flight writes
  int committed = -1;              // the one of the last accepted deskewed frame (-1: none)
  double xi[6] = {0, 0, 0, 0, 0, 0};   // the frame in flight's motion
  int64_t frames = 0, last_frame = -1;
  double last_twist[6] = {0, 0, 0, 0, 0, 0};
  void clear() { frames = 0; last_frame = -1; committed = -1; for (double& v : last_twist) v = 0.0; }
};

// place recognition (tl_api_place.hip): its configuration, the keyframe database in HBM (per keyframe the
// descriptor, both keys, the pose, the frame number; the loop records, at most one per keyframe, and their count), the search's
// scratch, the bins of the descriptor in flight (zero between descriptors), the storage a growth replaced (freed when the frame has
// drained the stream), and the buffers of tloam_place_add_scan / _describe
struct PlaceState {
  tloam_place_config cfg = {0, 20, 60, 10, 50, 0, 80.0, 2.0, 1.0, 0.2, 0.30, 0};   // tloam_place_default_config
  DBuf<double> desc, rkey, skey, pose, kdist;
  DBuf<long long> frame;
  DBuf<int> taken;
  DBuf<tloam_place_loop> loops;
  Retired retired;
  DBuf<unsigned long long> bins, ctl;   // ctl[0]: the number of loop records
  DBuf<PlaceCandidate> cand;
  DBuf<double> s_aos, s_desc, s_rkey, s_skey;
  size_t cap = 0;                  // keyframes the database holds
  int64_t n_kf = 0;
  int64_t last_kf_frame = -1;
  double last_pose[16];            // the last keyframe's pose (n_kf > 0)
  bool in_flight = false;          // a frame's place launches may still be reading its scan
  // loop verification on (tl_api_loop.hip): every keyframe's eight clouds in one arena (AoS, grown by
  // doubling through Grower, the old storage into `retired`), and the host's table of the keyframes -- frame number, pose, and
  // (offset, count) of each cloud -- so that nothing about them has to be read back
  struct Keyframe {
    int64_t frame;
    double pose[16];
    size_t off[8], n[8];   // [side * 4 + kind]: side 0 the source clouds, 1 the target clouds; off in doubles
  };
  std::vector<Keyframe> kf;        // [n_kf], kept whether or not verification is on
  DBuf<double> arena;
  size_t arena_used = 0;           // doubles
  tl::LoopSpanArgs pend;           // the frame in flight's eight spans (pend.nspan 0: none), committed with its keyframe
  void clear(hipStream_t s) {   // the run's keyframes and loops go; the configuration and storage stay
    n_kf = 0;
    last_kf_frame = -1;
    kf.clear();
    arena_used = 0;
    pend.nspan = 0;
    if (ctl.p) (void)hipMemsetAsync(ctl.p, 0, sizeof(unsigned long long), s);   // (behind whatever is in flight)
  }
};

// loop verification (tl_api_loop.hip): its configuration, the two private child contexts of the coarse and
// the fine stage (created lazily, on the parent's device), the verified constraints, the next loop record to verify, scratch
struct LoopState {
  tloam_loop_config cfg{};   // (zero: off)
  bool cfg_set = false;            // tloam_loop_configure has been called (else tloam_loop_default_config's, off)
  tloam_ctx* coarse = nullptr;
  tloam_ctx* fine = nullptr;
  std::vector<tloam_loop_constraint> out;
  size_t next_record = 0;
  DBuf<double> tgt, partial;       // the assembled targets (per kind, end to end), the score's block partials
  void clear() { out.clear(); next_record = 0; }
};

// pose-graph optimisation of the keyframes (tl_api_graph.hip): its configuration, the solver's device
// storage (doubles and integers, carved per call; grow-only), and the corrected keyframe poses of the last tloam_graph_optimize
struct GraphState {
  tloam_graph_config cfg = {30, 20000, 1e-7, 1e-10, 0.05, 0.005, 0.05, 0.01};   // tloam_graph_default_config
  DBuf<double> dws;
  DBuf<int> iws;
  DBuf<tl::GraphRecord> rec;
  bool have = false;               // tloam_graph_optimize has run since the last reset / configure
  std::vector<double> corrected;   // [16 n] column-major
  // the robust mode: its configuration (off), k_graph_reweight's record, and of the last optimise what it
  // reports, the loop edges' constraint indices, scales and statistics
  tloam_graph_robust_config rcfg = {0, 100, 36.0, 1.4};   // tloam_graph_robust_default_config
  DBuf<tl::GraphRobustRecord> rrec;
  tloam_graph_robust_info rinfo{};
  std::vector<int64_t> loop_constraint;
  std::vector<double> loop_scale, loop_chi2;
  void drop() {
    have = false;
    corrected.clear();
    rinfo = {};
    loop_constraint.clear(); loop_scale.clear(); loop_chi2.clear();
  }
};

// the closed map (tl_api_cmap.hip): its configuration, its rows in id order and their table (the voxel map's
// layout: k_vmap_read / k_vmap_box read them), what the last build reports and the poses it used, the reads' scratch.  A build's
// staging is its own and freed when it ends
struct CmapState {
  tloam_closed_map_config cfg = {1.0, {0.0, 0.0, 0.0}, 0xF0, 0, 0};   // tloam_closed_map_default_config until configured
  VoxelRowStore rows;
  bool built = false;              // a build has succeeded since the last drop
  bool detached = false;           // the map was loaded from a snapshot without its clouds: it cannot be built,
                                   // carved or surfelled again until it is emptied
  tloam_closed_map_info info{};    // of the last build (zero when dropped; capacity_voxels filled in when asked)
  std::vector<double> poses;       // [16 K] column-major: the poses the last build used
  DBuf<double> rd_c;
  DBuf<long long> rd_n;
  DBuf<unsigned long long> look, ctl;
  // the scratch of one scan-form call (cmap_scan_call below: a linearise, a diff, a ray-cast, an occupancy query) and of the free
  // space's other reads: a byte and an id per point, the control words (kDiffCtl: the largest user's).  Every call that uses
  // them waits for its read-back before it returns, so no two users are ever live at once and nothing is read after the call
  DBuf<unsigned char> scan_u8;
  DBuf<int> scan_ids;
  DBuf<unsigned long long> scan_ctl;
  // the carve (tl_api_carve.hip): its configuration, M in id order beside the rows, what the last carve
  // reports, the carved read's scratch.  The counts belong to the closed map they were counted in and go with it
  tloam_closed_map_carve_config carve_cfg = {60.0, 1.0, 0.25, 0, 0};   // tloam_closed_map_carve_default_config until configured
  DBuf<unsigned long long> miss, carve_ctl;
  DBuf<unsigned char> rd_m;        // (a box read's own columns are scratch in bytes: BoxColumn)
  bool carved = false;             // a carve has succeeded since the last drop
  tloam_closed_map_carve_info carve_info{};
  void drop_carve() {
    carved = false;
    carve_info = tloam_closed_map_carve_info{};
    free.drop_fields();            // the clearance and the frontiers may have been built under the gate (DESIGN.md sections 30, 32)
  }
  // the surfels (tl_api_surfel.hip): their configuration, the thirteen sums, the normals and the variances
  // in id order beside the rows (allocated by the first pass, for the rows' capacity), what the last pass reports, the box read's
  // scratch.  They belong to the closed map they were gathered in and go with it; a carve does not touch them
  tloam_closed_map_surfel_config surfel_cfg = {5, 0};   // tloam_closed_map_surfel_default_config until configured
  DBuf<unsigned long long> surfel_sums, surfel_ctl;
  DBuf<double> surfel_nrm, surfel_ev;
  DBuf<unsigned char> rd_nrm, rd_ev;
  DBuf<int> surfel_over;
  bool surfeled = false;           // a surfel pass has succeeded since the last drop
  tloam_closed_map_surfel_info surfel_info{};
  // the localisation (tl_api_localise.hip): its configuration, the voxel records {c, n, eligible} cached
  // beside the rows (allocated by the first call, for the rows' capacity; rebuilt when the surfels or the gate change), the
  // uploaded scan, the blocks' partial rows, the residuals of a linearise (its ids: scan_ids), the state words and the log of the
  // last call
  tloam_closed_map_localise_config loc_cfg = {1.0, 0.7, 0.1, HUGE_VAL, 0.05, 1e-6, 1e-7, 1e-9, 20, 50};   // _localise_default_config
  DBuf<tl::LocRecord> loc_rec;
  DBuf<double> loc_pts, loc_partial, loc_res;
  DBuf<tl::LocState> loc_state;
  DBuf<tl::LocLog> loc_log;
  bool loc_ready = false;          // the records are those of the surfels and the gate at hand
  std::vector<tloam_closed_map_localise_record> loc_records;   // of the last localise call
  // the batched localiser and the relocalisation on top of it: per hypothesis the log of the last batch
  // (or relocalise), the relocalisation's configuration, its candidates, hypotheses and the build's poses on the device, and the
  // hypotheses of the last relocalise
  std::vector<std::vector<tloam_closed_map_localise_record>> loc_batch_records;
  tloam_closed_map_relocalise_config reloc_cfg = {8, 0, HUGE_VAL, 0.5, HUGE_VAL};   // _relocalise_default_config
  DBuf<tl::PlaceCandidate> reloc_cand;
  DBuf<tl::RelocHyp> reloc_hyp;
  DBuf<double> reloc_poses;
  std::vector<tloam_closed_map_relocalise_hypothesis> reloc_hyps;
  void drop_localise() {
    loc_ready = false;
    loc_records.clear();
    loc_batch_records.clear();
    reloc_hyps.clear();
  }
  void drop_surfels() {
    surfeled = false;
    surfel_info = tloam_closed_map_surfel_info{};
    drop_localise();
  }
  // the diff of a scan against the map (tl_api_diff.hip): its configuration, through and hits in id order
  // beside the rows, what the last diff reports, the gone read's scratch.  The scan is uploaded where the localiser's is
  // (loc_pts), the labels read the localiser's records (loc_rec) and go through the scan-form scratch (scan_u8, scan_ids).  The
  // counts belong to the closed map they were counted in and go with it; a carve or a surfel pass does not touch them
  tloam_closed_map_diff_config diff_cfg = {60.0, 1.0, 0.25, 0.1, 0.5, 3, 1.0, 0, 0};   // tloam_closed_map_diff_default_config
  DBuf<unsigned long long> diff_through, diff_hits;
  DBuf<unsigned char> rd_through, rd_hits;
  bool diffed = false;             // a diff has succeeded since the last drop: there are counts
  tloam_closed_map_diff_info diff_info{};
  void drop_diff() {
    diffed = false;
    diff_info = tloam_closed_map_diff_info{};
  }
  // the ray-cast (tl_api_raycast.hip): its configuration, the ranges of the last call (its statuses and
  // ids: scan_u8, scan_ids) and what the last cast reports.  The ends are uploaded where the localiser's scan is (loc_pts) and
  // the tests read the localiser's records (loc_rec).  Nothing else is stored
  tloam_closed_map_raycast_config raycast_cfg = {120.0, 0.75, 1, 3, 1.0, 1, 0};   // tloam_closed_map_raycast_default_config
  DBuf<double> raycast_range;
  tloam_closed_map_raycast_info raycast_info{};
  void drop_raycast() { raycast_info = tloam_closed_map_raycast_info{}; }
  // the extension (tl_api_extend.hip): what the last extend of this map reports
  tloam_closed_map_extend_info extend_info{};
  // the free space (tl_api_free.hip): its configuration, the grid of brick words and its box, what the
  // grid reports, the cells read's scratch (the other reads': scan_u8, scan_ids, scan_ctl).  The grid belongs to the closed map it was gathered beside and goes with it (its memory
  // too: it can be large); an extend leaves it alone
  struct FreeState {
    tloam_closed_map_free_config cfg = {60.0, 1.0, (int64_t)1 << 30, 1, 3, 1.0, 0, 0};   // tloam_closed_map_free_default_config
    DBuf<unsigned long long> words, ctl, look;   // ctl: an add's counters (cmap_pass, cmap_scan_call)
    DBuf<double> rd_c;
    tl::FreeGrid grid{};
    bool have = false;             // a reset has succeeded since the last drop
    tloam_closed_map_free_info info{};
    // the clearance (tl_api_clear.hip): its configuration, the field and the buffer its passes alternate
    // with, what the last build reports, a segment call's starts and outputs and a column call's two layers (grow-only scratch;
    // the other outputs: scan_u8).  The field belongs to the grid and the map it was built from: whatever changes either drops it
    struct ClearState {
      tloam_closed_map_clearance_config cfg;   // tloam_closed_map_clearance_default_config until configured
      ClearState() { tloam_closed_map_clearance_default_config(&cfg); }
      DBuf<unsigned short> d2, tmp, out_u16, col_a, col_b;
      DBuf<double> starts, out_f64;
      tl::ClearField field{};
      bool have = false;           // a build has succeeded since the last drop
      tloam_closed_map_clearance_info info{};
      // the route (tl_api_route.hip): its configuration, the cost field with its two arrays of tile flags
      // and the control words of a build, what the last build reports, a query's outputs and a column call's layer (grow-only
      // scratch).  The field belongs to the clearance field it was built from and goes with it
      struct RouteState {
        tloam_closed_map_route_config cfg;   // tloam_closed_map_route_default_config until configured
        RouteState() { tloam_closed_map_route_default_config(&cfg); }
        DBuf<unsigned> cost, flags, out_u32, col_cost, col_flags;
        DBuf<unsigned long long> ctl;
        DBuf<int> out_i32;
        DBuf<double> out_f64;
        tl::TileField field{};
        bool have = false;           // a build has succeeded since the last drop
        tloam_closed_map_route_info info{};
        void drop() {
          have = false;
          info = tloam_closed_map_route_info{};
          field = tl::TileField{};
          cost.release();            // (hipFree waits for the launches that use them)
          flags.release();
        }
      } route;
      void drop() {
        have = false;
        info = tloam_closed_map_clearance_info{};
        field = tl::ClearField{};
        d2.release();              // (hipFree waits for the launches that use them)
        tmp.release();
        route.drop();
      }
    } clear;
    // the frontiers (tl_api_frontier.hip): their configuration, the label field with its two arrays of
    // tile flags, the cluster table (roots, records, the kept list's records, a component's kept index) and the look-back words
    // of its compactions, the control words, what the last build reports and its kept list on the host, a query's outputs and a
    // column call's own field and table (grow-only scratch).  The field belongs to the grid and the map's counting voxels, not to
    // the clearance: whatever changes either drops it (drop_fields below), the clearance's and the route's calls leave it alone
    struct FrontierState {
      tloam_closed_map_frontier_config cfg;   // tloam_closed_map_frontier_default_config until configured
      FrontierState() { tloam_closed_map_frontier_default_config(&cfg); }
      struct Bufs {
        DBuf<unsigned> label, flags, roots;
        DBuf<tloam_closed_map_frontier_cluster> rec, kept_rec;
        DBuf<int> kept_of;
        DBuf<unsigned long long> look;
        void release() { label.release(); flags.release(); roots.release(); rec.release(); kept_rec.release(); kept_of.release(); look.release(); }
      } own, col;
      DBuf<unsigned long long> ctl, keys;
      DBuf<unsigned> out_u32;
      DBuf<int> out_i32;
      DBuf<double> out_f64;
      tl::TileField field{};
      tl::FrontTable table{};
      std::vector<tloam_closed_map_frontier_cluster> kept;   // the kept list as the build read it back
      bool have = false;           // a build has succeeded since the last drop
      tloam_closed_map_frontier_info info{};
      // the view gain (tl_api_view.hip): its configuration, the uploaded poses, the records, the views'
      // beyond-window counts, the global form's windows and counters, the cells form's centres (grow-only scratch) and what the
      // last call reports.  It reads the field as the dense state array of the box: nothing is stored, the info goes with the field
      struct ViewState {
        tloam_closed_map_view_config cfg;   // tloam_closed_map_view_default_config until configured
        ViewState() { tloam_closed_map_view_default_config(&cfg); }
        DBuf<double> poses, out_f64;
        DBuf<tloam_closed_map_view_record> rec;
        DBuf<unsigned long long> beyond, cnt;
        DBuf<unsigned> win;
        tloam_closed_map_view_info info{};
      } view;
      void drop() {
        have = false;
        info = tloam_closed_map_frontier_info{};
        view.info = tloam_closed_map_view_info{};
        field = tl::TileField{};
        table = tl::FrontTable{};
        kept.clear();
        own.release();             // (hipFree waits for the launches that use them)
        view.win.release();
      }
    } frontier;
    // what was built from the grid and the map's counting voxels goes when either changes: the one list
    void drop_fields() {
      clear.drop();
      frontier.drop();
    }
    void drop() {
      have = false;
      info = tloam_closed_map_free_info{};
      grid = tl::FreeGrid{};
      words.release();             // (hipFree waits for the launches that use it)
      drop_fields();
    }
  } free;
  void drop() {   // the closed map goes, and the carve's counts, the surfels, the diff's counts, the last ray-cast's info and the free-space
                  // grid with it; the configurations and storage stay
    built = false;
    detached = false;
    info = tloam_closed_map_info{};
    extend_info = tloam_closed_map_extend_info{};
    poses.clear();
    drop_carve();
    drop_surfels();
    drop_diff();
    drop_raycast();
    free.drop();
  }
};

// up to four SoA clouds (x, y, z, n) a search grid is built over -- the registered targets, or any other cloud
struct CloudRef { const double *x, *y, *z; size_t n; };
}  // namespace tlh

using namespace tlh;

struct tloam_ctx {
  tloam_tls_config cfg;
  SubmapState submap;
  FeatBuffers feat;
  SegBuffers seg;
  OdomState odom;
  MapState map;
  VmapState vmap;
  DeskewState deskew;
  PlaceState place;
  LoopState loop;
  GraphState graph;
  CmapState cmap;
  int device = 0;
  hipStream_t stream = nullptr;
  KindData kd[kKinds];
  // concatenated per-source-slot arrays of the current scan_match
  DBuf<double> sx, sy, sz, w_src, raw;
  DBuf<double> fit_x, fit_y, fit_z;  // getFitnessScore scratch
  DBuf<unsigned long long> flags, scan, scan_tmp, tile_cnt, tile_scan;
  DBuf<unsigned long long> scan1p_q;   // control words of the single-pass scan of the query-sort histogram, zero when allocated
  bool scan1p_q_use = false;           // ... and whether this frame's query sort takes it (reserve_query_sort: scan_path on this device)
  bool grids_ahead = false;    // the search grids in `grids_next` were built over the registered targets at hand-over (tloam_set_target_frame) and are still theirs
  // ... which is also CHECKED: every path that changes a registered target cloud advances tgt_gen, the grids built ahead remember
  // the generation they were built over, and tloam_sm_begin swaps them in only if that is still the current one
  unsigned long long tgt_gen = 0, grids_next_gen = ~0ull;
  bool no_grid_ahead = false;  // TLOAM_NO_GRID_AHEAD: the grids are always built inside scanMatching (A/B, tests)
  bool no_scan_1p = false;     // set after a single-pass look-back scan timed out (blocks not co-resident): the multi-launch scans from then on
  DBuf<unsigned char> flagb;   // SlotView::flagb
  DBuf<double> fin_rows;       // hand-over rows of the finish riding on a thread-per-query search (k_build_finish_large)
  bool fused_large = false;    // TLOAM_FUSED_LARGE: a GN iteration of a large set as ONE launch (k3_sweep_step; sharded + mailbox: sweep, exchange
                               // and step).  Measured slower than sweep + step as two launches: off by default
  DBuf<int> tile_of_slot, tile_fill;
  DBuf<double4> qrec;  // tile-sorted query records (x, y, z, slot)
  GridBuffers grids;  // the four search grids of the last scanMatching (shared buffers)
  GridBuffers grids_knn;       // ... the grid of the last tloam_knn (its own radius; kept, so that a query batch allocates nothing)
  tloam_grid_info grid_info = {};   // the last grid build of any of them (tloam_get_grid_info)
  GridBuffers grids_next;      // ... and the set built AHEAD, over targets just handed over (tloam_set_target_frame); swapped in by the next sm_begin
  tl::GridView gv_next[tl::kKinds];
  SlotView sv{};
  CorrView cv{};
  DBuf<int> seg_n;
  DBuf<double> partials, red48, sums16, wpart, rank_counts, se3_dev, bbox_dev, misc;
  DBuf<GnState> state;
  Pinned<GnState> h_state;     // pinned mirror
  Pinned<double> h_small;      // pinned scratch (>= 64*6*4 doubles)
  int k3_grid = 1;
  bool k3_single = false;
  bool k3_wide = false;        // the streaming sweep goes out as blocks of eight waves (k3_plan); k3_grid = blocks launched = rows
  int dbg_max_sweeps = 0;          // development knobs, read from the environment once at create
  bool dbg_no_build_reuse = false;
  bool dbg_no_eval_reuse = false;
  bool no_device_loop = false;     // TLOAM_NO_DEVICE_LOOP: tloam_scan_match keeps the host in the outer loop (A/B, tests)
  bool no_persistent_solve = false;  // TLOAM_NO_PERSISTENT_SOLVE, or set by tloam_scan_match after an in-launch hand-over timed out:
                                     // KITTI-size Solves run one launch per GN iteration instead of k_solve_all
  bool hand_over_timed_out = false;  // the last TLOAM_E_HIP of the device loop was OS_COMM_ERROR on one rank
  int dbg_fail_handover = 0;       // TLOAM_DEBUG_FAIL_HANDOVER=n: the next n one-launch Solves time out in their first hand-over (test hook)
  int device_cus = 0;              // multiProcessorCount of the device (k_solve_all and the single-pass scans need all their blocks resident at once)
  Pinned<double> h_bbox;           // pinned, device-visible: [4][64][6] bounding-box rows
  // bounds of the registered target clouds, taken at hand-over (set_target*: the call synchronises anyway), so that
  // scanMatching can size its search grids without a host round trip of its own
  double tgt_box[tl::kKinds][6];
  bool tgt_box_valid[tl::kKinds] = {false, false, false, false};
  double wait_us = 0.0;            // time the host spent waiting for the device in the current scan_match
  double hs[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // development aid (TLOAM_HOST_STAMPS): where the calling thread's time goes, per frame
  long hs_n = 0;
  double hs_exit = 0.0;
  double hs_entry = 0.0;          // > 0: stamping, entry time of the scan_match in progress (us, steady clock)
  Pinned<tl::MirrorSlot> h_mirror;          // pinned, device-visible result slots (HostMirror targets), 64-byte aligned
  unsigned long long mirror_seq = 0;
  // fault words a kernel raises when a bounded in-launch wait runs out (pinned, device-visible; see check_device_faults):
  // [0] single-pass look-back scan (tl_nn.hip), [1] k_vox_emit's look-back (tl_submap.hip)
  Pinned<unsigned> h_fault;
  bool scan1p_retried = false;     // tloam_scan_match has re-run a frame after a look-back scan timed out (once per context)
  bool vox_ticket = false;         // set after k_vox_emit's look-back timed out: its blocks take start tickets from then on
  DBuf<double> src_pack;                        // the registered Frame's four source clouds in one piece (tloam_set_source_frame)
  // pinned staging of tloam_set_source_frame: the borrowed host clouds are copied here (two halves, used alternately; an
  // event per half says when the device has read it) and go to HBM with ONE asynchronous copy -- the call returns without
  // waiting for the device, the frame's first kernel is ordered behind the copy by the stream
  Pinned<double> h_stage[2];                    // (.dev: the halves as the device addresses them, for kernels that read the
                                                //  staging in place; .n: doubles)
  hipEvent_t stage_ev[2] = {nullptr, nullptr};
  bool stage_busy[2] = {false, false};
  int stage_next = 0;
  std::vector<std::unique_ptr<tlh::FrameClouds>> frame_store;   // tloam_frame_stash / tloam_frame_select
  int frame_selected = -1;                      // slot whose clouds are the registered ones (-1: the context's own)
  int dbg_planned_sweeps = 0;      // TLOAM_PLANNED_SWEEPS: force the sweep budget per Solve (exercises the top-up)
  std::vector<int> planned_sweeps; // per outer iteration x 3: sweeps the Solve needed in the last three frames
  bool prebuilt = false;
  // comm
  int rank = 0, nranks = 1;
  CommMode comm = COMM_NONE;
  // A mailbox or RCCL set-up with nranks == 1: the context exchanges with ITSELF -- every launch of the sharded forms runs (fused
  // sweep + post, gather + step, the side exchanges), the exchange is a loop-back, the results are those of the single-rank forms
  // bit for bit (one row folded onto +0.0).  What times the sharded forms at shard size on ONE GPU (bench: shard_size_iterations)
  // and makes a one-rank RCCL communicator actually carry the all-reduce (tests/test_gpu_multirank.py)
  bool loopback = false;
  tloam_allreduce_fn cb = nullptr;
  void* cb_user = nullptr;
  void* nccl_comm = nullptr;
  // one-shot peer exchange (tl_common.hpp MboxView): the local buffer (fine-grained device memory, exported through
  // HIP IPC), the peers' buffers as mapped here, the device-resident exchange counter, the ticket of the fused sweep
  double* mbox_local = nullptr;
  void* mbox_opened[tl::kMaxRanks] = {};   // hipIpcOpenMemHandle results (closed at destroy: comm_release, like mbox_local)
  tl::MboxView mbox{};
  DBuf<unsigned long long> mbox_ctr;
  DBuf<int> k3_ticket;
  DBuf<unsigned long long> k3_span;    // K3Step::span: streaming span of the one-launch GN iterations (100 MHz ticks, launches)
  DBuf<unsigned long long> iter_span;  // iter_span_note (tl_gn.hip): [0] last stamp, [1] ticks, [2] periods; handed to the kernels once
  bool iter_timing = false;            // tloam_gn_iter_timer has armed it
  // bounded in-launch waits that ran out on this context (look-back scan, voxel look-back, one-launch Solve hand-over): every
  // one moved the context to a form that waits for nothing -- tloam_get_info reports which, and how often
  int fallback_events = 0;
  bool persistent_solve_timed_out = false;   // no_persistent_solve was set by a time-out, not by TLOAM_NO_PERSISTENT_SOLVE
  // the DIRECT factor set of large frames (tl_common.hpp DirectSet): chosen per frame by tloam_sm_begin
  bool no_qbin_ride = false;   // TLOAM_NO_QBIN_RIDE: the query sort's first pass as a launch of its own (A/B)
  bool qbin_rode = false;      // this frame's query binning rode on the grid build (launch_build skips its own)
  bool no_direct_set = false;  // TLOAM_NO_DIRECT_SET: large frames compact as the others do (A/B, tests)
  // The launch forms of the frame (tl_forms.hpp), written where a factor set's shape becomes known: tloam_sm_begin (and its
  // demotion of a direct frame without a grid for every kind) and tloam_set_correspondences.  The knobs that only select forms --
  // no_persistent_solve, no_direct_set, no_device_loop, fused_large, no_qbin_ride -- reach the driver through forms_in alone
  // (dbg_no_build_reuse too, but it also changes what tloam_sm_outer does inside the host-driven loop).
  // forms.set == DIRECT: rows = tile-sorted queries, holes, two weight streams
  tl::FrameForms forms;
  bool set_stale = false;      // a direct set's rows hold the geometry of a search whose set was never solved (OS_SET_STALE): rebuilt at
                               // x_build before a getter reads them
  int w_parity = 0;            // weight stream the CURRENT GNC weights are in (the captured ones of the last Solve: the other)
  DBuf<GnState> state_scratch; // a copy of the state with T_cur = exp(x_build), for that rebuild
  DBuf<int> row_of_pos;        // DirectSet::row_of_pos: the row of every sorted query position
  DBuf<int> fin_tickets;       // FinishDirect::ticket: the top ticket + one per group of 64 finish blocks (zero between launches)
  DBuf<int> blk_cnt;           // DirectSet::blk_cnt: [2 parities][search blocks][4]
  size_t blk_cnt_n = 0;        // search blocks of this frame
  // scanMatching host state
  bool active = false;
  bool have_build = false;   // the compact set matches build_x
  double build_x[6] = {0, 0, 0, 0, 0, 0};
  int iter = 0;
  double mu = 1.0, noise_bound_sq = 1e-4;
  double prev_cost[kKinds], cur_cost[kKinds];
  tloam_stats stats;
  // K3 timing (bench roofline)
  bool k3_timing = false;
  std::vector<hipEvent_t> ev_pool;
  size_t ev_used = 0;
  std::vector<int> ev_batch_idx;   // position of each sampled launch inside its batch (solve)
  int batch_launches = 0;          // K3 launches enqueued since the last harvest
  long long k3_seq = 0;            // all K3 launches of this context
  double k3_total_us = 0.0, k3_all_us = 0.0;  // working sweeps only / every K3 launch incl. no-ops
  int64_t k3_launches = 0, k3_all_launches = 0;
  double k3_alg_bytes = 0.0;  // algorithmic bytes of ONE sweep over the current set
  std::string last_error;
};

#define HIPC(ctx, expr)                                                                 \
  do {                                                                                  \
    hipError_t _e = (expr);                                                             \
    if (_e != hipSuccess) {                                                             \
      (ctx)->last_error = std::string(#expr) + ": " + hipGetErrorString(_e);            \
      return TLOAM_E_HIP;                                                               \
    }                                                                                   \
  } while (0)

// pinned result slots: one per outer iteration of a device-driven frame (slot 0: stepwise API); the last one also
// carries the sizes of a submap update back (tl_api_submap.hip)
constexpr int kMirrorSlots = tl::kResultSlots;
constexpr int kFaultWords = 16;
constexpr int kFaultScan1p = 0, kFaultVoxEmit = 1;   // tloam_ctx::h_fault
// Points a single cloud / correspondence set / query batch may hold: slots, cells and ranks are 32-bit integers throughout, and the
// four kinds of a frame share one slot space -- 2^28 points (6.4 GB as doubles) per cloud keeps every sum over the four kinds
// (<= 2^30) and every 3 n inside it (2^29 did not: four clouds at the bound sum to INT_MAX + 1).  Sums that grow behind the
// entry points -- a submap's accumulated clouds -- are checked where they are formed (submap_update_body).
// More is TLOAM_E_INVALID at the entry point, not an overflow behind it.
constexpr size_t kMaxPoints = (size_t)1 << 28;

namespace tlh {
// ---- small helpers shared by the API units
// column-major 4x4 products, sums over k in ascending order, and Eigen::Isometry3d::inverse (R^T, -R^T t): the odometry's
// prediction, loop verification's T_rel and the pose graph's Z round alike (their units are compiled with -ffp-contract=off)
// the steady clock in microseconds: the TLOAM_HOST_STAMPS brackets
static inline double host_now_us() {
  return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
static inline void mat_mul(const double A[16], const double B[16], double out[16]) {
  double r[16];
  for (int j = 0; j < 4; ++j)
    for (int i = 0; i < 4; ++i) r[4 * j + i] = ((A[i] * B[4 * j] + A[4 + i] * B[4 * j + 1]) + A[8 + i] * B[4 * j + 2]) + A[12 + i] * B[4 * j + 3];
  memcpy(out, r, sizeof(r));
}
static inline void rigid_inverse(const double T[16], double out[16]) {
  double r[16];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) r[4 * j + i] = T[4 * i + j];
    r[12 + i] = -((T[4 * i] * T[12] + T[4 * i + 1] * T[13]) + T[4 * i + 2] * T[14]);
    r[4 * i + 3] = 0.0;
  }
  r[15] = 1.0;
  memcpy(out, r, sizeof(r));
}
inline double kind_radius(const tloam_tls_config& c, int k) {
  switch (k) {
    case TLOAM_KIND_PLANAR: return c.planar_dist_thres;
    case TLOAM_KIND_GROUND: return c.ground_dist_thres;
    case TLOAM_KIND_EDGE: return c.edge_dist_thres;
    default: return c.sphere_dist_thres;
  }
}
inline int kind_maxnum(const tloam_tls_config& c, int k) {
  switch (k) {
    case TLOAM_KIND_PLANAR: return c.planar_maxnum;
    case TLOAM_KIND_GROUND: return c.ground_maxnum;
    case TLOAM_KIND_EDGE: return c.edge_maxnum;
    default: return c.sphere_maxnum;
  }
}
// registration.cpp:979-1016: factor_num 4 -> all four builders, 3 -> planar+ground+edge, 2 -> planar+ground
inline int kind_active(const tloam_tls_config& c, int k) {
  if (c.factor_num == 4) return 1;
  if (c.factor_num == 3) return k != TLOAM_KIND_SPHERE;
  if (c.factor_num == 2) return k == TLOAM_KIND_PLANAR || k == TLOAM_KIND_GROUND;
  return 0;
}
inline size_t round_up(size_t v, size_t m) { return (v + m - 1) / m * m; }
// what a configure entry point is asked for: *cfg, or what its default_config fills in when cfg is null
template <class Cfg>
Cfg cfg_or_default(const Cfg* cfg, void (*default_fn)(Cfg*)) {
  Cfg want;
  if (cfg) want = *cfg;
  else default_fn(&want);
  return want;
}
// a list getter over a host vector (the caller has checked n): *n is the list's length, whatever follows; the list is copied
// when `out` is given and holds it.  A null `out` or an empty list is TLOAM_OK, a short capacity TLOAM_E_INVALID
template <class T>
int copy_list(const std::vector<T>& list, size_t capacity, size_t* n, T* out) {
  *n = list.size();
  if (!out || list.empty()) return TLOAM_OK;
  if (capacity < list.size()) return TLOAM_E_INVALID;
  memcpy(out, list.data(), sizeof(T) * list.size());
  return TLOAM_OK;
}

// `fresh` holds `want` rows, the first `keep` of `cur` copied into it device to device on the stream
template <class T>
hipError_t grow_into(DBuf<T>& fresh, const DBuf<T>& cur, size_t want, size_t keep, hipStream_t s) {
  hipError_t e = fresh.reserve(want);
  if (e == hipSuccess && keep) e = hipMemcpyAsync(fresh.p, cur.p, sizeof(T) * keep, hipMemcpyDeviceToDevice, s);
  return e;
}

// One growth of a store, all its arrays or none: add() gives an array fresh storage of `want` rows behind whatever is in flight,
// the first `keep` rows copied (0: the array is rebuilt, not copied), and returns it (nullptr once anything failed); commit()
// swaps every fresh array in and parks the old storage in the store's Retired -- or, after a failure, frees the fresh arrays,
// leaves the store as it was and returns TLOAM_E_HIP with `what` in last_error.  Until then the fresh arrays are the Grower's
class Grower {
 public:
  Grower(tloam_ctx* c, Retired& parked) : c_(c), parked_(parked) {}
  template <class T>
  T* add(DBuf<T>& cur, size_t want, size_t keep = 0) {
    if (e_ != hipSuccess) return nullptr;
    DBuf<T> fresh;
    e_ = grow_into(fresh, cur, want, keep, c_->stream);
    T* const q = fresh.p;
    if (q) {
      arrays_.push_back({&cur, fresh.cap, &swap_in<T>});
      fresh_.take(fresh);
    }
    return e_ == hipSuccess ? q : nullptr;
  }
  void check(hipError_t e) {   // a step on the fresh storage (the first failure counts)
    if (e_ == hipSuccess) e_ = e;
  }
  int commit(const char* what) {
    if (e_ != hipSuccess) {
      (void)hipStreamSynchronize(c_->stream);
      fresh_.release();
      c_->last_error = std::string(what) + hipGetErrorString(e_);
      return TLOAM_E_HIP;
    }
    for (size_t i = 0; i < arrays_.size(); ++i) arrays_[i].swap(arrays_[i].cur, fresh_.p[i], arrays_[i].cap, parked_);
    fresh_.p.clear();   // (the store's now)
    return TLOAM_OK;
  }

 private:
  struct Array {
    void* cur;     // the store's DBuf<T>
    size_t cap;    // of its fresh storage, fresh_.p[same index]
    void (*swap)(void* cur, void* fresh, size_t cap, Retired& parked);
  };
  template <class T>
  static void swap_in(void* cur, void* fresh, size_t cap, Retired& parked) {
    DBuf<T>& b = *static_cast<DBuf<T>*>(cur);
    parked.take(b);
    b.p = static_cast<T*>(fresh);
    b.cap = cap;
  }
  tloam_ctx* c_;
  Retired& parked_;
  hipError_t e_ = hipSuccess;
  std::vector<Array> arrays_;
  Retired fresh_;   // the fresh arrays are the Grower's until commit() hands them to the store (freed with it otherwise)
};
inline bool one_rank(const tloam_ctx* c) { return c->nranks == 1 && !c->loopback; }    // the single-rank launch forms apply
inline bool exchanging(const tloam_ctx* c) { return c->nranks > 1 || c->loopback; }    // the sharded launch forms run
// tl_api_comm.hip
int allreduce(tloam_ctx* c, double* dev, int count);   // sum all-reduce of a small device buffer of doubles across the context's ranks
void comm_release(tloam_ctx* c);
void comm_rccl_info(const tloam_ctx* c, int32_t* count, int32_t* user_rank);   // ncclCommCount / ncclCommUserRank of the context's communicator, -1 without one
// tl_api_match.hip
int reserve_seg(tloam_ctx* c, int k, size_t n);        // compact correspondence segment of kind k for n factors
int ensure_common(tloam_ctx* c);                       // the context's small fixed device buffers
int reserve_query_sort(tloam_ctx* c, const tl::GridView grids[tl::kKinds]);   // the buffers of the frame's query sort, sized by the grids
int reserve_tile_hist(tloam_ctx* c, size_t ntiles, bool frame_start, size_t* room = nullptr);   // ... its histogram and scan: the one size rule
tl::FormsIn forms_in(const tloam_ctx* c);              // what decide_forms looks at, from the context (every kind assumed to get a grid)
// ... and what tl_api_sets.hip shares with the frame:
constexpr int kSolveSweeps = 5;                        // max_num_iterations 4 -> at most 1 + 4 evaluations per Solve
tl::BuildParams build_params(const tloam_ctx* c);      // the search's radii, caps and active kinds from the configuration
void outer_params(const tloam_ctx* c, tl::BuildParams* bp, tl::GridView grids[tl::kKinds]);   // ... and the frame's four grids
void plan_sweeps(tloam_ctx* c);                        // k3_grid / k3_single / k3_wide from the segments' capacities
int reserve_partials(tloam_ctx* c);                    // the sweeps' per-block rows for k3_grid
double* direct_w_stream(const tloam_ctx* c, int k, int parity);   // weight stream `parity` of kind k's direct rows
double alg_bytes_of(const int n[tl::kKinds]);          // algorithmic bytes of one sweep over n factors per kind
int launch_k3_timed(tloam_ctx* c, bool force);         // one streaming sweep, sampled by the K3 timer when it is armed
int harvest_k3_events(tloam_ctx* c, int working);      // ... its samples folded into the timers after one Solve of `working` sweeps
int enqueue_solve(tloam_ctx* c, bool armed, int sweeps, const tl::WeightParams* wp = nullptr, const tl::SolvePrep* prep = nullptr,
                  const tl::SolveFinish* finish = nullptr);   // one ceres::Solve on the current set, device resident
// tl_api_frames.hip
void exchange_clouds(tloam_ctx* c, FrameClouds& F);    // the registered clouds <-> a FrameClouds (pointers and counts only)
int check_device_faults(tloam_ctx* c);
int wait_word(tloam_ctx* c, const unsigned long long* p, unsigned long long seq);
int wait_segment(tloam_ctx* c, const unsigned long long* seg, unsigned long long seq, unsigned long long payload[7]);
// After the frame's last wait: the payload of the stage segment the frame in flight posted as number `pending` (0: none posted,
// nothing to collect: returns 1), in pinned memory already -- read, not waited for.  Should the stream have drained without it,
// `device_words(pay)` copies the stage's own device words into `pay` and synchronises, returning the bytes it copied or a status
template <class DeviceWords>
int collect_segment(tloam_ctx* c, const PinnedSeg& seg, unsigned long long& pending, tloam_odom_stats* st,
                    unsigned long long pay[7], DeviceWords device_words) {
  if (!pending) return 1;
  const int rc = wait_segment(c, seg.h, pending, pay);
  if (rc < 0) return rc;
  if (rc != TLOAM_OK) {   // (the stream has drained and the segment is not there: the device words)
    const int bytes = device_words(pay);
    if (bytes < 0) return bytes;
    st->d2h_bytes += bytes;
    st->host_syncs++;
  }
  st->d2h_bytes += 8 * (int64_t)sizeof(unsigned long long);   // the segment
  pending = 0;
  return TLOAM_OK;
}
int stage_and_upload(tloam_ctx* c, const double* const parts[], const size_t counts[], int nparts, double* dev_dst, size_t offs[]);
int stage_in_place(tloam_ctx* c, const double* const parts[], const size_t counts[], int nparts, size_t offs[], const double** dev_view,
                   int* half);
int stage_release(tloam_ctx* c, int half, bool completed);
size_t staged_size(const size_t counts[], int nparts);
size_t staged_offsets(const size_t counts[], int nparts, size_t offs[]);   // where staging puts the pieces; returns the total
int source_frame_reserve(tloam_ctx* c, const size_t n[4], size_t cnt4[4]);
void source_frame_commit(tloam_ctx* c, bool ok, const size_t off[4]);
int set_target_copy(tloam_ctx* c, int kind, const double* xyz, size_t n, hipMemcpyKind from);
// tl_api_seg.hip: tloam_segment as "begin" (count the call, size the buffers), upload into seg.aos, "launch"
bool seg_config_ok(const tloam_seg_config& cfg);
int segment_begin(tloam_ctx* c, const tloam_seg_config& cfg, size_t n, tl::SegParams* out);
int segment_launch(tloam_ctx* c, const tl::SegParams& P);
// tl_api_feature.hip: calculatePCAInfo / the ranking of extractPlanarSphere on the cloud resident in feat.aos
int feature_reserve(tloam_ctx* c, const tloam_feature_config& cfg, size_t n, FeatBuffers& F);
int feature_pca_run(tloam_ctx* c, const tloam_feature_config& cfg, size_t n, FeatBuffers& F, tl::FeatArgs* out);
int feature_select_launch(tloam_ctx* c, const tloam_feature_config& cfg, size_t n, FeatBuffers& F, const tl::FeatArgs& A);
// tl_api_submap.hip
bool submap_config_ok(const tloam_submap_config& cfg);
int submap_init_body(tloam_ctx* c, const tloam_submap_config& want, const double* planar, size_t n_planar, const double* sphere,
                     size_t n_sphere, const double* edge, size_t n_edge, const double* ground, size_t n_ground, hipMemcpyKind from);
int submap_update_resident(tloam_ctx* c, const double pose[16], size_t n_planar, size_t n_sphere, size_t n_edge, size_t n_ground,
                           DBuf<double>& block);
// tl_api_map.hip: the odometry frame's map stage -- reserve at the start of a later frame, launch after the match, collect the
// count after the frame's last wait, commit when the frame is accepted
int map_frame_reserve(tloam_ctx* c, size_t n);
int map_stage_launch(tloam_ctx* c, const double pose[16], size_t n);
int map_stage_collect(tloam_ctx* c, tloam_odom_stats* st);
void map_frame_end(tloam_ctx* c, bool accepted);
// tl_api_vmap.hip: the merged voxel map's stage, at the same four points of the frame
int vmap_frame_reserve(tloam_ctx* c, size_t n);
int vmap_stage_launch(tloam_ctx* c, const double pose[16], size_t n);
int vmap_stage_collect(tloam_ctx* c, tloam_odom_stats* st);
void vmap_frame_end(tloam_ctx* c, bool accepted);
// tl_api_vmap.hip: the one read path of voxel rows -- the merged voxel map's and the closed map's (k_vmap_read and the three box
// kernels).  What a read needs of either state: the rows as the kernels see them, the reads' scratch, the voxels held, the
// errors' name
struct VoxelRows {
  tl::VmapReadArgs base;
  DBuf<double>& rd_c;
  DBuf<long long>& rd_n;
  DBuf<unsigned long long>& look;
  DBuf<unsigned long long>& ctl;
  size_t nv;
  const char* name;
};
template <class State>
VoxelRows voxel_rows_of(State& S, size_t nv, const char* name) {
  tl::VmapReadArgs A;
  memset(&A, 0, sizeof(A));
  A.map = S.rows.view();
  A.voxel = S.cfg.voxel;
  for (int a = 0; a < 3; ++a) A.origin[a] = S.cfg.origin[a];
  return VoxelRows{A, S.rd_c, S.rd_n, S.look, S.ctl, nv, name};
}
// ids [first, first + count) to the host; the caller has checked its context (and that a closed map is built)
int voxel_rows_read(tloam_ctx* c, const VoxelRows& R, size_t first, size_t count, double* centroids_aos, int64_t* counts);
// The host half of a box read: the voxels of the box (null: the whole map) with N >= min_count that the kernel keeps, in id
// order, to the host.  `launch` is handed the filled rows (scratch reserved, look and ctl zeroed) and enqueues `kernel`, named
// in the timeout's message; `extra` are the read's own columns beside the centroids and the counts
struct BoxColumn {
  void* host;                 // where the caller wants it (null: not asked for)
  DBuf<unsigned char>* dev;   // the column's device scratch, in bytes
  size_t per_voxel, elem;     // elements per voxel, bytes per element
};
template <class Launch>
int voxel_rows_read_box(tloam_ctx* c, const VoxelRows& R, const double* lo, const double* hi, int64_t min_count, size_t capacity,
                        size_t* n, double* centroids_aos, int64_t* counts, const char* kernel, std::initializer_list<BoxColumn> extra,
                        Launch launch) {
  const size_t nv = R.nv;
  if (nv == 0) return TLOAM_OK;
  HIPC(c, hipSetDevice(c->device));
  HIPC(c, hipStreamSynchronize(c->stream));   // (the scratch may be replaced)
  const size_t blocks = (nv + 255) / 256;
  HIPC(c, R.rd_c.reserve(3 * nv)); HIPC(c, R.rd_n.reserve(nv));
  for (const BoxColumn& x : extra) HIPC(c, x.dev->reserve(x.per_voxel * x.elem * nv));
  HIPC(c, R.look.reserve(blocks + 1)); HIPC(c, R.ctl.reserve(8));
  HIPC(c, hipMemsetAsync(R.look.p, 0, sizeof(unsigned long long) * (blocks + 1), c->stream));
  HIPC(c, hipMemsetAsync(R.ctl.p, 0, sizeof(unsigned long long) * 8, c->stream));
  tl::VmapReadArgs A = R.base;
  A.first = 0; A.count = nv;
  for (int a = 0; a < 3; ++a) { A.lo[a] = lo ? lo[a] : 0.0; A.hi[a] = hi ? hi[a] : 0.0; }
  A.min_count = min_count;
  A.out_c = R.rd_c.p; A.out_n = R.rd_n.p;
  A.look = R.look.p; A.ctl = R.ctl.p;
  launch(A);
  HIPC(c, hipGetLastError());
  unsigned long long w[3];
  HIPC(c, hipMemcpyAsync(w, R.ctl.p, sizeof(w), hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  if (w[1]) {
    c->last_error = std::string(R.name) + ": a look-back of " + kernel + " timed out";
    return TLOAM_E_HIP;
  }
  const size_t m = (size_t)w[2];
  *n = m;
  if (m == 0) return TLOAM_OK;
  if (capacity < m) return TLOAM_E_INVALID;
  const hipMemcpyKind D2H = hipMemcpyDeviceToHost;
  if (centroids_aos) HIPC(c, hipMemcpyAsync(centroids_aos, R.rd_c.p, sizeof(double) * 3 * m, D2H, c->stream));
  if (counts) HIPC(c, hipMemcpyAsync(counts, R.rd_n.p, sizeof(int64_t) * m, D2H, c->stream));
  for (const BoxColumn& x : extra)
    if (x.host) HIPC(c, hipMemcpyAsync(x.host, x.dev->p, x.per_voxel * x.elem * m, D2H, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  return TLOAM_OK;
}
// tl_api_cmap.hip: the closed map's span table for `mask` over keyframes [first, min(K, kf.size())): keyframes ascending, a
// keyframe's selected clouds in slot order, empty clouds left out, the end sentinel (spans->back().start = *n) last; a span's kf
// counts from `first` (the poses and flags beside the table are those keyframes' alone); *empty_keyframes (may be null) counts the
// keyframes that add no span
void cmap_span_table(const PlaceState& P, size_t first, size_t K, int mask, std::vector<tl::CmapSpan>* spans, long long* n,
                     int64_t* empty_keyframes);
// ... and its device copy beside the K poses, a stage's own: freed with it (hipFree waits for the launches that use them)
struct SpanUpload {
  DBuf<tl::CmapSpan> span;
  DBuf<double> pose;
  // both uploaded on the context's stream; *in: what the kernels take (arena, span, nspan, nkf, n, pose)
  int upload(tloam_ctx* c, const std::vector<tl::CmapSpan>& spans, long long n, const double* poses, size_t K, tl::SpanInput* in);
};
// the built closed map as its stages look voxels up in it: every Work's `grid`
inline tl::MapGrid map_grid_of(const CmapState& M) {
  tl::MapGrid G;
  memset(&G, 0, sizeof(G));
  G.voxel = M.cfg.voxel;
  for (int a = 0; a < 3; ++a) G.origin[a] = M.cfg.origin[a];
  G.map = M.rows.view();
  G.nv = (long long)M.info.n_voxels;
  return G;
}
// One pass over the points the closed map was built from (the carve, the surfels): the span table for `mask` over the build's
// keyframes uploaded beside the build's poses, the fields every pass's Work has filled (in, grid, ctl), the
// launches of fill_and_launch(W), which fills the rest and returns their number, the eight words of `ctl` read back, one wait.
// reserve() sizes the pass's arrays, `ctl` among them, after waiting when one that it replaces may still be read.  `first`: the
// pass runs over keyframes [first, K) alone (the free space's add after an extension): their spans, their poses
struct CmapPassOut {
  unsigned long long ctl[8];
  size_t K;        // the build's keyframes: later ones add nothing
  long long n;     // the points of all spans
  int launches;
};
template <class Work, class Reserve, class Launch>
int cmap_pass(tloam_ctx* c, int mask, const DBuf<unsigned long long>& ctl, Reserve reserve, Launch fill_and_launch, CmapPassOut* out,
              size_t first = 0) {
  const CmapState& M = c->cmap;
  out->K = M.poses.size() / 16;
  first = std::min(first, out->K);
  std::vector<tl::CmapSpan> spans;
  cmap_span_table(c->place, first, out->K, mask, &spans, &out->n, nullptr);
  HIPC(c, hipSetDevice(c->device));
  int rc = reserve();
  if (rc != TLOAM_OK) return rc;
  SpanUpload up;   // the pass's own, freed with it
  Work W;
  memset(&W, 0, sizeof(W));
  rc = up.upload(c, spans, out->n, M.poses.data() + 16 * first, out->K - first, &W.in);
  if (rc != TLOAM_OK) return rc;
  W.grid = map_grid_of(M);
  W.ctl = ctl.p;
  out->launches = fill_and_launch(W);
  HIPC(c, hipGetLastError());
  HIPC(c, hipMemcpyAsync(out->ctl, ctl.p, sizeof(out->ctl), hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  return TLOAM_OK;
}
// ... and its public entry point: the context and the built map checked, the previous result dropped (from there on a failure
// leaves none), body(I) run, the stream drained when it fails (nothing of the pass is in flight when its span table goes), its
// info and flag committed when it succeeds
template <class Info, class Body>
int cmap_pass_entry(tloam_ctx* c, void (CmapState::*drop)(), Info CmapState::*last, bool CmapState::*ran, Info* info, Body body) {
  if (!c || c->nranks > 1) return TLOAM_E_INVALID;
  CmapState& M = c->cmap;
  if (!M.built) return TLOAM_E_NOT_READY;
  (M.*drop)();
  Info I;
  memset(&I, 0, sizeof(I));
  const int rc = body(I);
  if (rc != TLOAM_OK) {
    (void)hipStreamSynchronize(c->stream);
    return rc;
  }
  M.*last = I;
  M.*ran = true;
  if (info) *info = I;
  return TLOAM_OK;
}
// ids [first, first + count) of a side array of the built closed map (`ran`: the stage that fills it has run): TLOAM_OK when the
// range is one
int cmap_side_range(const tloam_ctx* c, bool ran, size_t first, size_t count);
// what tloam_closed_map_load (tl_api_snapshot.hip) needs of the units whose state it installs: their configure's own tests of a
// configuration, and the room a default configuration reserves
bool place_config_valid(const tloam_place_config& cfg);             // tl_api_place.hip
size_t place_default_reserve();
bool loop_config_valid(const tloam_loop_config& cfg);               // tl_api_loop.hip
bool cmap_config_valid(const tloam_closed_map_config& cfg);         // tl_api_cmap.hip
size_t cmap_default_reserve();
bool carve_config_valid(const tloam_closed_map_carve_config& cfg);  // tl_api_carve.hip
// tl_api_free.hip, for the clearance built from the grid (tl_api_clear.hip): the context and the grid checked for a call that
// needs one, the same for a read (which resolves occupancy: the gate needs the carve's counts), and what a read resolves it with
int free_ready(const tloam_ctx* c);
int free_read_ready(const tloam_ctx* c);
tl::FreeQuery free_query(const CmapState& M);
// tl_api_localise.hip: the localiser's voxel records {c, n, eligible} sized and, when they are stale, their rebuild enqueued
// (*prepared = 1; k_loc_prepare).  cmap_scan_call sets CmapState::loc_ready once the call that asked for them has succeeded
int loc_records_prepare(tloam_ctx* c, int* prepared);
// `pose` (column-major) is finite and a rigid transform: what every call that takes a live scan at a pose asks of it, after its
// argument and readiness checks (TLOAM_E_INVALID when not).  *T (may be null): the pose as pose_from_matrix forms it.
// (static: each includer's own copy, rounded under its own flags.)
static inline bool pose_finite_rigid(const double* pose, tl::Pose* T = nullptr) {
  for (int i = 0; i < 16; ++i)
    if (!(pose[i] - pose[i] == 0.0)) return false;
  tl::Pose rigid;
  return tl::pose_from_matrix(pose, T ? T : &rigid);
}
// One scan-form call on the built closed map -- a live scan (or segment ends) at a pose, queried against the map: the localiser's
// runs and its linearise, the diff, the ray-cast, the free space's add_scan and occupancy -- the counterpart of cmap_pass for
// keyframe passes.  In order: the device set; the stream waited for once when a buffer about to grow is too small (the stream is
// idle at entry of these synchronous calls: it costs nothing in steady state); loc_pts, the control words and whatever
// rooms(room) names through room(buffer, elements) reserved; the scan uploaded; the localiser's records prepared when
// `records` (*prepared); the control words zeroed; fill_and_launch(grid, scan), which fills the rest of its Work, launches and
// returns a status; hipGetLastError; the control words read back into ctl_out; the caller's reads() enqueued; one wait.
// A failure drains the stream and, when the records were involved, marks them stale; the caller then drops what it must
// (drop_diff, free.drop()).  On success with records, loc_ready is set.
struct CmapScanCall {
  const double* points_aos;          // the scan, AoS, sensor frame
  size_t n;
  const double* pose;                // column-major, taken as it stands (null: none, scan.M is zero)
  bool records;                      // the call reads the localiser's voxel records
  DBuf<unsigned long long>* ctl;     // the control words (null: none) ...
  size_t n_ctl;                      // ... their number, zeroed before the launches
  unsigned long long* ctl_out;       // [n_ctl] as the launches left them
};
template <class Rooms, class Launch, class Reads>
int cmap_scan_call(tloam_ctx* c, const CmapScanCall& q, int* prepared, Rooms rooms, Launch fill_and_launch, Reads reads) {
  CmapState& M = c->cmap;
  auto body = [&]() -> int {
    HIPC(c, hipSetDevice(c->device));
    auto all_rooms = [&](auto room) -> int {
      HIPC(c, room(M.loc_pts, 3 * q.n));
      if (q.ctl) HIPC(c, room(*q.ctl, std::max<size_t>(q.n_ctl, tl::kDiffCtl)));   // (the largest user's: never regrown)
      return rooms(room);
    };
    bool grows = false;
    (void)all_rooms([&](auto& buf, size_t n) { grows = grows || buf.cap < n; return hipSuccess; });
    if (grows) HIPC(c, hipStreamSynchronize(c->stream));   // (what is replaced may still be read)
    int rc = all_rooms([](auto& buf, size_t n) { return buf.reserve(n); });
    if (rc != TLOAM_OK) return rc;
    HIPC(c, hipMemcpyAsync(M.loc_pts.p, q.points_aos, sizeof(double) * 3 * q.n, hipMemcpyHostToDevice, c->stream));
    *prepared = 0;
    if (q.records && (rc = loc_records_prepare(c, prepared)) != TLOAM_OK) return rc;
    if (q.ctl) HIPC(c, hipMemsetAsync(q.ctl->p, 0, sizeof(unsigned long long) * q.n_ctl, c->stream));
    tl::ScanAt scan;
    memset(&scan, 0, sizeof(scan));
    scan.pts = M.loc_pts.p;
    scan.n = (long long)q.n;
    if (q.pose) memcpy(scan.M, q.pose, sizeof(scan.M));   // the matrix as it stands
    rc = fill_and_launch(map_grid_of(M), scan);
    if (rc != TLOAM_OK) return rc;
    HIPC(c, hipGetLastError());
    if (q.ctl) HIPC(c, hipMemcpyAsync(q.ctl_out, q.ctl->p, sizeof(unsigned long long) * q.n_ctl, hipMemcpyDeviceToHost, c->stream));
    rc = reads();
    if (rc != TLOAM_OK) return rc;
    HIPC(c, hipStreamSynchronize(c->stream));
    return TLOAM_OK;
  };
  const int rc = body();
  if (rc != TLOAM_OK) (void)hipStreamSynchronize(c->stream);   // nothing of the call stays in flight
  if (q.records) M.loc_ready = rc == TLOAM_OK;                  // (a failed call's records are rebuilt by the next)
  return rc;
}
// the field over box B, its lowest cell at `lo`, its words at v
inline tl::TileField field_of(const tlt::TileBox& B, const int lo[3], unsigned* v) {
  tl::TileField f;
  memset(&f, 0, sizeof(f));
  f.v = v;
  for (int a = 0; a < 3; ++a) { f.lo[a] = lo[a]; f.n[a] = (int)B.n[a]; f.tiles[a] = (int)B.tiles[a]; }
  f.cells = (long long)B.cells;
  return f;
}
// The rounds of a tiled field (tl_tile.hpp: the route's costs, the frontiers' labels) after its seed has flagged the first
// round's tiles in flags[0 .. ntiles) (flags[ntiles .. 2 ntiles) zero): batches of min(rounds_per_wait, what max_rounds leaves)
// launches of launch_round(f, now, next, marks, stream), `now` and `next` swapped after each, round k of a batch counting its
// fresh marks into ctl_rounds[k] (zero before the first batch by the caller's memset, zeroed here before every later one); the
// batch's counters read back -- with the first batch also head[0 .. n_head) from head_dev, what the seed counted -- and one wait a
// batch.  The first round that marked nothing ends it: the rounds after it found no flag up.  When max_rounds are enqueued and
// none has: last_error "<who>: the <noun> had not settled after max_rounds = ..." and TLOAM_E_HIP.  On a failure launches may
// be in flight: the caller drains the stream.
struct TileRounds {
  int64_t rounds, enqueued, updates;   // rounds counted up to the first that marked nothing, launches enqueued, tiles marked
  int waits;
};
template <class Launch>
int tile_rounds(tloam_ctx* c, const char* who, const char* noun, int64_t max_rounds, int64_t rounds_per_wait, const tl::TileField& f,
                unsigned* flags, size_t ntiles, unsigned long long* ctl_rounds, Launch launch_round, const unsigned long long* head_dev,
                unsigned long long* head, size_t n_head, TileRounds* out) {
  unsigned* now = flags;            // the seed's marks are the first round's tiles
  unsigned* next = flags + ntiles;
  unsigned long long marks[tl::kTileMaxBatch];
  *out = TileRounds{};
  bool done = false;
  while (!done) {
    const int batch = (int)std::min<int64_t>(rounds_per_wait, max_rounds - out->enqueued);
    if (batch <= 0) {
      c->last_error = std::string(who) + ": the " + noun + " had not settled after max_rounds = " + std::to_string(max_rounds) + " rounds";
      return TLOAM_E_HIP;
    }
    if (out->enqueued) HIPC(c, hipMemsetAsync(ctl_rounds, 0, sizeof(unsigned long long) * batch, c->stream));
    for (int k = 0; k < batch; ++k) {
      launch_round(f, now, next, ctl_rounds + k, c->stream);
      std::swap(now, next);
    }
    HIPC(c, hipGetLastError());
    if (!out->enqueued) HIPC(c, hipMemcpyAsync(head, head_dev, sizeof(unsigned long long) * n_head, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipMemcpyAsync(marks, ctl_rounds, sizeof(unsigned long long) * batch, hipMemcpyDeviceToHost, c->stream));
    HIPC(c, hipStreamSynchronize(c->stream));
    ++out->waits;
    out->enqueued += batch;
    for (int k = 0; k < batch && !done; ++k) {
      ++out->rounds;
      out->updates += (int64_t)marks[k];
      done = marks[k] == 0ull;   // a round that marked nothing: the rounds after it found no flag up
    }
  }
  return TLOAM_OK;
}
// tl_api_deskew.hip: the frame's deskew -- sized and its times uploaded after the scan's upload, launched after the segmentation's
// (the refused-time flag read with the frame's first wait), committed when the frame ends
int deskew_frame_upload(tloam_ctx* c, const double* t_sec, size_t n, tloam_odom_stats* st);
int deskew_frame_launch(tloam_ctx* c, size_t n, unsigned long long* bad_host, tloam_odom_stats* st);
void deskew_frame_end(tloam_ctx* c, bool accepted, int64_t frame);
// the frame's scan as its stages after the segmentation read it: the deskewed copy when the frame corrected it
inline const double* frame_scan(const tloam_ctx* c) { return c->deskew.active ? c->deskew.aos.p : c->seg.aos.p; }
// tl_api_place.hip: place recognition -- the database grown at the start of a frame; an accepted keyframe described, committed
// and searched by launches enqueued after the frame's last wait
int place_frame_reserve(tloam_ctx* c, size_t n);
void place_frame_end(tloam_ctx* c, bool accepted, int64_t frame, const double pose[16], const double* scan, size_t n);
// loop verification on: room in the keyframe cloud arena for the frame's eight clouds (after the frame's wait 3: nothing is
// waited for), then the eight spans noted for place_frame_end's k_place_clouds (spans 0-3 the source kinds, 4-7 the target kinds)
bool place_clouds_on(const tloam_ctx* c);
int place_clouds_reserve(tloam_ctx* c, const size_t n[8]);
void place_clouds_note(tloam_ctx* c, const tl::LoopSpan spans[8]);
int arena_grow(tloam_ctx* c, size_t need_doubles);   // (tl_api_place.hip) the arena holds arena_used + need doubles
void loop_release(tloam_ctx* c);                      // (tl_api_loop.hip) at destroy / off: the child contexts, the scratch
// (tl_api_graph.hip) what tloam_graph_correct_pose computes, after its checks of the context: P'_k * rigid_inverse(P_k) * pose_in
void graph_correct_pose(const tloam_ctx* c, size_t keyframe, const double pose_in[16], double pose_out[16]);
int set_target_frame_from(tloam_ctx* c, const double* const xyz[4], const size_t n[4], hipMemcpyKind from);   // tl_api_frames.hip
int voxel_down_sample_launch(tloam_ctx* c, const size_t n[2], const double voxel[2], int nseg, double* const out[2][3]);
int build_grids_over(tloam_ctx* c, GridBuffers& G, const double radius[tl::kKinds], const CloudRef clouds[tl::kKinds],
                     tl::GridView out[tl::kKinds], const double (*known_boxes)[6] = nullptr,
                     tl::FrameInitHook* frame = nullptr);
int build_grids(tloam_ctx* c, GridBuffers& G, const double radius[tl::kKinds], tl::GridView out[tl::kKinds],
                tl::FrameInitHook* frame = nullptr);
void reduce_box_rows(const double* box_rows, double boxes[tl::kKinds][6]);   // rows of k_bbox_all / k_ingest_targets -> (lo, hi) per kind
int enqueue_target_bounds(tloam_ctx* c);
void finish_target_bounds(tloam_ctx* c);
}  // namespace tlh
